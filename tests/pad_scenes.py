"""Padded bitmap fill scenes ("Padded bitmap fills") and their libcairo reference: FadeReplay -- so that "blend_mode",
"layer", "mask" and "opacity" mean what they mean in the other families -- over a backend whose set_fill_pattern can ask for
CAIRO_EXTEND_PAD (cairo_extend_t 3) on the surface pattern of a fill that carries "pad".

tools/make_pad_goldens.py writes goldens() to tests/golden/cairo_pad_*.npz (premultiplied RGBA; key = scene name); the tests rebuild
the scenes from here, so a golden file holds pixels only.  Frames are 96 x 48 and one of 300 x 40 (five tile columns, three tile-rows).

The bitmaps are 1 x 1, 2 x 2, 3 x 5 and 8 x 8, every texel its own colour (so all four edges and all four corners differ).  A
DefineBitmap tag (image/x-swf-bmp, format 3) has an opaque palette, so translucent edge texels come from a colour transform -- the
variant texture of the `cxform` file, whose alpha multiplier makes every texel translucent -- and from random_box_case, whose texels are
registered as straight RGBA (swfr_register_bitmap) with translucent ones among them.

The `cxform` files stay out of files(), the list of what goes through every device route: swfr_build_frame's arrays of such a frame
name textures of the handle that walked the stage, so they cannot be handed to another handle (tests/device_routes.py,
built_for_another_handle).  tests/test_pad_gpu.py takes them through all five routes too, with swfr_build_frame called on the drawing
handle where a route wants arrays.
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
import fade_scenes as fs  # noqa: E402
import mask_scenes as ms  # noqa: E402
from scenarios import _m, _poly_shape  # noqa: E402

LINEAR_BOUND = fs.LINEAR_BOUND               # (no scene here has a linear gradient: everything is exact)
golden_path = bs.golden_path
W, H = 96, 48
CAIRO_EXTEND = {"none": 0, "repeat": 1, "pad": 3}      # cairo_extend_t
EXTENDS = ("none", "repeat", "pad")


# ---- the libcairo reference
def _backend(width, height):
    from oracle import cairo_backend as cb

    class PadBackend(cb.CairoBackend):
        """CairoBackend whose surface patterns get cairo_pattern_set_extend(self.extend) where that is set: 3 is CAIRO_EXTEND_PAD"""
        extend = None

        def set_fill_pattern(self, bitmap, repeat):
            super().set_fill_pattern(bitmap, repeat)
            if self.extend is not None:
                self._fill = self._fill[:2] + (self.extend,)
    return PadBackend(width, height)


class PadReplay(fs.FadeReplay):
    """FadeReplay that hands a padded fill's extend to the backend before the path is drawn.  The decoded path keeps the fill's
    "repeating" as it stands in the tag, so for_cairo() writes "pad" there (still truthy) for a fill that carries "pad"."""

    def _draw_path(self, path):
        self.be.extend = CAIRO_EXTEND["pad"] if path.get("fill", {}).get("repeating") == "pad" else None
        return super()._draw_path(path)


def for_cairo(obj):
    """a copy of the tree in which every bitmap fill with a truthy "pad" says "repeating": "pad" (what PadReplay reads)"""
    if isinstance(obj, list):
        return [for_cairo(o) for o in obj]
    if isinstance(obj, dict):
        out = {k: for_cairo(v) for k, v in obj.items()}
        if out.get("type") == "bitmap" and out.get("pad"):
            assert not out.get("repeating")
            out["repeating"] = "pad"
        return out
    return obj


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a pad scene through libcairo; sc["raw_bitmaps"]: id -> (width, height, straight RGBA bytes)"""
    be = _backend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        low = ms._lowering(sc.get("bitmaps", []))
        stage = low.lower(for_cairo(sc["stage"]))
        rp = PadReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        for bid, (w, h, px) in list(low.extra.items()) + list(sc.get("raw_bitmaps", {}).items()):
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def with_extend(obj, extend):
    """the same tree with the edge rule of every bitmap fill replaced: "none", "repeat" or "pad" """
    if isinstance(obj, list):
        return [with_extend(o, extend) for o in obj]
    if isinstance(obj, dict):
        out = {k: with_extend(v, extend) for k, v in obj.items() if not (k == "pad" and obj.get("type") == "bitmap")}
        if out.get("type") == "bitmap":
            out["repeating"] = extend == "repeat"
            if extend == "pad":
                out["pad"] = True
        return out
    return obj


# ---- pieces
SIZES = {11: (1, 1), 12: (2, 2), 13: (3, 5), 14: (8, 8)}         # bitmap id -> (width, height)


def _tag(bid):
    """a DefineBitmap (image/x-swf-bmp, format 3) whose texels all have colours of their own"""
    w, h = SIZES[bid]
    rng = np.random.default_rng(100 + bid)
    table = np.zeros((w * h, 3), np.uint8)
    seen = set()
    for k in range(w * h):
        while True:
            c = tuple(int(v) for v in rng.integers(0, 256, 3))
            if c not in seen:
                break
        seen.add(c)
        table[k] = c
    padded = w + (-w) % 4
    idx = np.zeros((h, padded), np.uint8)
    idx[:, :w] = np.arange(w * h).reshape(h, w)
    data = bytes([3, w & 255, w >> 8, h & 255, h >> 8, w * h - 1]) + zlib.compress(table.tobytes() + idx.tobytes())
    return {"type": "define-bitmap", "id": bid, "width": w, "height": h, "media_type": "image/x-swf-bmp", "data": data.hex()}


BITMAPS = [_tag(bid) for bid in sorted(SIZES)]


def _fill(bid, matrix, extend="pad"):
    f = {"type": "bitmap", "bitmap_id": bid, "repeating": extend == "repeat", "smoothed": True, "matrix": matrix}
    if extend == "pad":
        f["pad"] = True
    return f


def _at(kx, ky, x, y, r0=0.0, r1=0.0):
    """the fill matrix that draws a texel kx x ky pixels large, the bitmap's corner at pixel (x, y); r0, r1: skew, in pixels per texel"""
    return _m(20 * kx, 20 * ky, round(x * 20), round(y * 20), 20 * r0, 20 * r1)


def _shape(pts_px, fill, **kw):
    return {"type": "shape", "definition": _poly_shape([(round(x * 20), round(y * 20)) for x, y in pts_px], fill), **kw}


def _box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _quad(x0, y0, x1, y1):
    """a slanted quadrilateral (in pixels) inside the rectangle: antialiased edges all round"""
    return [(x0 + 1.3, y0 + 0.4), (x1 - 0.6, y0 + 1.7), (x1 - 2.2, y1 - 0.3), (x0 + 0.2, y1 - 1.6)]


def _scene(kids, w=W, h=H):
    return dict(width=w, height=h, exact=True, bitmaps=BITMAPS, stage={"children": kids})


GROUND = [bs._shape([(3.3, 2.6), (W - 2.2, 4.1), (W - 5.4, H - 3.2), (1.7, H - 6.3)], (60, 140, 220, 150))]


def _fitted(bid, k, x, y):
    """a shape that is exactly the bitmap's rectangle, the bitmap k times magnified with its corner at (x, y): what the authoring tool
    places on the stage"""
    w, h = SIZES[bid]
    return _shape(_box(x, y, x + k * w, y + k * h), _fill(bid, _at(k, k, x, y)))


# ---- the groups
def fit_scenes():
    """every bitmap as a shape of exactly its own rectangle, 1 x, 2.5 x and 7.75 x magnified side by side, at integer and at fractional
    offsets; the 8 x 8 one also cut by the frame's lower edge"""
    out = {}

    def row(bid, ox, oy):
        kids, x = [], ox
        for k in (1, 2.5, 7.75):
            kids.append(_fitted(bid, k, x, oy))
            x += k * SIZES[bid][0] + 2.25
        return kids
    for oname, (ox, oy) in (("integer", (1, 2)), ("fractional", (1.35, 2.6))):
        # (a 1 x 1 bitmap looks the same padded and repeated: it shares its frames with the 3 x 5 one)
        out["fit_3x5_1x1_%s" % oname] = _scene(row(13, ox, oy) + row(11, ox + 44, oy + 3))
        out["fit_2x2_%s" % oname] = _scene(row(12, ox, oy))
        out["fit_8x8_%s" % oname] = _scene(row(14, ox, oy))
    out["fit_over_ground"] = _scene(GROUND + [_fitted(13, 7.75, 8.4, 3.3), _fitted(12, 7.75, 40.5, 20.25), _fitted(11, 7.75, 70.7, 9.9)])
    return out


def reach_scenes():
    """shapes that reach past the bitmap: on all four sides at once, past each side and each corner alone; a row of one wavefront's 64
    pixels that straddles the bitmap's edge and rows wholly outside it; coverage 255 with opaque texels; the three edge rules of one
    bitmap in one frame"""
    out = {}
    for bid, k, x, y in ((13, 3.5, 40.3, 14.6), (12, 6.25, 41.7, 17.2), (14, 2.5, 37.1, 13.3)):
        w, h = SIZES[bid]
        fill = _fill(bid, _at(k, k, x, y))
        out["beyond_all_%dx%d" % (w, h)] = _scene([_shape(_quad(2, 1, 94, 47), fill)])
        out["beyond_all_%dx%d_over_ground" % (w, h)] = _scene(GROUND + [_shape(_quad(2, 1, 94, 47), fill)])
    # (a 1 x 1 bitmap looks the same padded and repeated: it shares its frame with the 2 x 2 one)
    out["beyond_all_1x1_2x2"] = _scene([_shape(_quad(2, 1, 47, 47), _fill(11, _at(5.0, 5.0, 22.4, 20.9))), _shape(_quad(49, 1, 94, 47), _fill(12, _at(3.25, 3.25, 68.7, 20.2)))])
    # one shape per side and per corner of the 3 x 5 bitmap at 3.5 x (10.5 x 17.5 pixels at (40.3, 14.6)): each its own operation
    bid, k, x, y = 13, 3.5, 40.3, 14.6
    x1, y1 = x + 3 * k, y + 5 * k
    places = {"left": (x - 30.2, y + 3.1, x + 2.2, y1 - 2.4), "right": (x1 - 2.1, y + 2.2, x1 + 31.4, y1 - 3.3), "top": (x + 1.6, y - 12.3, x1 - 1.2, y + 3.1),
              "bottom": (x + 2.1, y1 - 2.7, x1 - 1.7, y1 + 13.2), "corner_tl": (x - 25.5, y - 11.1, x + 2.6, y + 2.9), "corner_tr": (x1 - 3.3, y - 12.4, x1 + 28.8, y + 2.2),
              "corner_bl": (x - 27.7, y1 - 2.8, x + 3.1, y1 + 12.6), "corner_br": (x1 - 2.4, y1 - 3.6, x1 + 26.3, y1 + 14.1)}
    for name, rect in places.items():
        out["beyond_" + name] = _scene([_shape(_quad(*rect), _fill(bid, _at(k, k, x, y)))])
    out["beyond_each_in_one_frame"] = _scene([_shape(_quad(*rect), _fill(bid, _at(k, k, x, y))) for rect in places.values()])
    # the 8 x 8 bitmap 4 x magnified at (30.3, 14.6): columns 30 .. 62 of a 92-pixel row, rows 2 .. 14 and 47 .. 48 wholly outside
    out["straddle_box"] = _scene([_shape(_box(2, 2, 94, 48), _fill(14, _at(4, 4, 30.3, 14.6)))])
    out["straddle_quad"] = _scene([_shape(_quad(0, 0, 96, 48), _fill(14, _at(4, 4, 30.3, 14.6)))])
    out["outside_rows_only"] = _scene([_shape(_box(3, 1, 90, 9), _fill(14, _at(4, 4, 30.3, 14.6))), _shape(_quad(1, 12, 26, 40), _fill(14, _at(4, 4, 30.3, 14.6)))])
    # the first paint of the frame lies wholly outside its bitmap: unpadded it would draw nothing and leave the surface clear, so the
    # translucent solid behind it would still be composited with the SOURCE rule; padded the surface has been drawn on
    out["outside_first_then_translucent"] = _scene([_shape(_box(3, 1, 90, 9), _fill(14, _at(4, 4, 30.3, 14.6))),
                                                    bs._shape([(5.5, 3.2), (88.3, 5.9), (40.1, 44.6)], (200, 20, 20, 100))])
    # coverage 255 everywhere, opaque texels: whole wavefronts take the "plain" shortcut
    out["full_coverage"] = _scene([_shape(_box(0, 0, 96, 48), _fill(13, _at(9, 6, 34, 9)))])
    # the three edge rules of one bitmap
    for bid, k in ((13, 2.5), (12, 1.75)):
        w, h = SIZES[bid]
        kids = [_shape(_quad(1 + 32 * i, 2, 31 + 32 * i, 46), _fill(bid, _at(k, k, 11.4 + 32 * i, 14.7), e)) for i, e in enumerate(("pad", "none", "repeat"))]
        out["together_%dx%d" % (w, h)] = _scene(kids)
    return out


def matrix_scenes():
    """rotated and skewed fill matrices, a mirrored one, an object matrix; minified below 0.75 (pixman's separable convolution) on one
    axis, on the other, on both, and rotated"""
    out = {}
    shape = lambda fill, **kw: _shape(_quad(2, 1, 94, 47), fill, **kw)
    c, s = np.cos(0.6), np.sin(0.6)
    out["rotated"] = _scene([shape(_fill(13, _m(20 * 4 * c, 20 * 4 * c, 900, 300, 20 * 4 * s, -20 * 4 * s)))])
    out["skewed"] = _scene([shape(_fill(14, _at(2.5, 1.75, 30.3, 12.2, 0.6, -0.9)))])
    out["mirrored"] = _scene([shape(_fill(13, _at(-3.25, 4.5, 52.6, 11.1)))])
    out["object_matrix"] = _scene([shape(_fill(12, _at(5, 5, 40.2, 16.4)), matrix=_m(0.9, 0.95, 90, 20, 0.04, -0.06))])
    out["rotated_over_ground"] = _scene(GROUND + [shape(_fill(12, _m(20 * 6 * c, 20 * 6 * c, 800, 500, -20 * 6 * s, 20 * 6 * s)))])
    out["minified_x"] = _scene([shape(_fill(14, _at(0.5, 3.0, 44.3, 10.7)))])
    out["minified_y"] = _scene([shape(_fill(14, _at(3.0, 0.4, 30.2, 20.6)))])
    out["minified_both"] = _scene([shape(_fill(14, _at(0.6, 0.45, 45.3, 21.7)))])
    out["minified_3x5_1x1"] = _scene([_shape(_quad(2, 1, 47, 47), _fill(13, _at(0.7, 0.3, 24.1, 22.4))), _shape(_quad(49, 1, 94, 47), _fill(11, _at(0.5, 0.5, 70.6, 23.3)))])
    out["minified_rotated"] = _scene([shape(_fill(14, _m(20 * 0.55 * c, 20 * 0.55 * c, 900, 400, 20 * 0.55 * s, -20 * 0.55 * s)))])
    out["minified_fit"] = _scene([_shape(_box(10.2, 8.4, 10.2 + 8 * 0.5, 8.4 + 8 * 0.5), _fill(14, _at(0.5, 0.5, 10.2, 8.4))),
                                  _shape(_box(30, 8, 30 + 3 * 0.6, 8 + 5 * 0.6), _fill(13, _at(0.6, 0.6, 30, 8)))])
    return out


def _padded_pair():
    """a magnified and a minified padded fill side by side, both reaching past their bitmaps"""
    return [_shape(_quad(2, 1, 50, 47), _fill(13, _at(3.5, 3.5, 20.3, 14.6))), _shape(_quad(46, 3, 94, 45), _fill(14, _at(0.6, 0.5, 66.2, 20.9)))]


def structure_scenes():
    """the padded pair under "blend_mode", "layer", "mask" and "opacity"; and the 300 x 40 frame of the two-band routes"""
    out = {}
    pair = _padded_pair()
    out["blend_mode"] = _scene(GROUND + [dict(p, blend_mode="multiply") for p in pair])
    out["layer"] = _scene(GROUND + [{"type": "container", "layer": "screen", "children": pair + [bs._rect(30, 8, 70, 30, (200, 20, 20, 100))]}])
    out["mask"] = _scene(GROUND + [{"type": "container", "children": pair, "mask": [bs._shape([(12.4, 6.3), (86.2, 9.8), (80.7, 40.1), (15.6, 43.6)], (10, 200, 90, 200))]}])
    out["opacity"] = _scene(GROUND + [{"type": "container", "opacity": 150, "children": pair + [bs._rect(30, 8, 70, 30, (200, 20, 20, 100))]}])
    out["wide"] = _scene([_shape(_quad(3, 1, 297, 39), _fill(14, _at(6.5, 3.25, 120.4, 6.6))), _shape(_quad(200, 4, 290, 36), _fill(13, _at(0.6, 0.6, 240.4, 18.6)))], 300, 40)
    return out


def cxform_scenes():
    """the padded pair under colour transforms -- variant textures: the texels are recoloured, the addressing stays -- one of which
    makes every texel, so every edge, translucent; and coverage 255 with opaque edge texels beside the same with translucent ones"""
    import make_cxform_goldens as mk
    out = {}
    tint = mk.cxform(mult=(256, 200, 128, 256), add=(0, 20, 60, 0))
    veil = mk.cxform(mult=(256, 230, 256, 150), add=(0, 0, 10, 0))
    out["cxform_tint"] = _scene(GROUND + [{"type": "container", "color_transform": tint, "children": _padded_pair()}])
    out["cxform_translucent"] = _scene(GROUND + [{"type": "container", "color_transform": veil, "children": _padded_pair()}])
    out["full_coverage_translucent_beside_opaque"] = _scene(GROUND + [
        _shape(_box(0, 0, 96, 24), _fill(13, _at(9, 3, 34, 6))),
        {"type": "container", "color_transform": veil, "children": [_shape(_box(0, 24, 96, 48), _fill(13, _at(9, 3, 34, 30)))]}])
    return out


GROUPS = {"fit": fit_scenes, "reach": reach_scenes, "matrices": matrix_scenes, "structure": structure_scenes}
CXFORM_GROUPS = {"cxform": cxform_scenes}


def all_scenes():
    out = {}
    for make in list(GROUPS.values()) + list(CXFORM_GROUPS.values()):
        out.update(make())
    return out


def _files(groups):
    return {"cairo_pad_%s%s" % ("aliased_" if aliased else "", group): (make, aliased) for aliased in (False, True) for group, make in groups.items()}


def files():
    """golden file name -> (scenes, aliased): what every device route must reproduce byte for byte"""
    return _files(GROUPS)


def cxform_files():
    """the same for the colour-transformed scenes (the module's docstring: not in files())"""
    return _files(CXFORM_GROUPS)


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())}
            for fname, (make, aliased) in dict(files(), **cxform_files()).items()}


# ---- random single boxes (tests/test_pad_model.py against libcairo, tests/test_pad_gpu.py against the model)
FW, FH = 32, 16
PLACES = ("inside", "rim", "outside")


def random_box_case(rng, minified=None):
    """One pixel-aligned box with a padded bitmap fill on a clear FW x FH frame: the frame then holds the source samples themselves.
    Bitmap 1 .. 9 texels per axis, straight RGBA with translucent texels among them; a matrix from 0.3 x to 12 x per axis with rotation
    (`minified`: True below 0.75 -- the convolution -- False at or above, None either); the box aimed inside the bitmap, across its rim
    or wholly outside it.  -> dict(scene, model=dict(matrices, bitmap (h, w, 4) straight RGBA, rect))"""
    bw, bh = int(rng.integers(1, 10)), int(rng.integers(1, 10))
    px = rng.integers(0, 256, (bh, bw, 4)).astype(np.uint8)
    px[..., 3] = np.where(rng.integers(0, 3, (bh, bw)) == 0, px[..., 3], 255)        # a third of the texels translucent
    aim = PLACES[int(rng.integers(0, 3))]
    if minified is None:
        minified = bool(rng.integers(0, 2))
    if minified:
        kx, ky = float(rng.uniform(0.3, 0.74)), float(rng.uniform(0.3, 3.0))
        if rng.integers(0, 2):
            kx, ky = ky, kx
    else:
        kx, ky = float(rng.uniform(0.76, 12.0)), float(rng.uniform(0.76, 12.0))
    if aim == "inside":                              # (a sample has to find all its taps inside: a large bitmap on the frame)
        bw, bh = max(bw, 6), max(bh, 6)
        px = np.resize(px, (bh, bw, 4))
        kx, ky = (max(kx, 0.5), max(ky, 0.5)) if minified else (max(kx, 3.0), max(ky, 3.0))
    t = float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 3) == 0 and aim != "inside" else 0.0
    c, s = np.cos(t), np.sin(t)
    sx, sy, r0, r1 = int(round(20 * kx * c * 65536)), int(round(20 * ky * c * 65536)), int(round(20 * kx * s * 65536)), int(round(-20 * ky * s * 65536))
    # the box, and the texel-space point that is to land on its centre
    w, h = (1, 1) if aim == "inside" else (int(rng.integers(1, 7)), int(rng.integers(1, 5)))
    x0, y0 = int(rng.integers(0, FW - w + 1)), int(rng.integers(0, FH - h + 1))
    if aim == "inside":
        u, v = bw / 2 + float(rng.uniform(-0.5, 0.5)), bh / 2 + float(rng.uniform(-0.5, 0.5))
    elif aim == "rim":
        u, v = [(0, rng.uniform(0, bh)), (bw, rng.uniform(0, bh)), (rng.uniform(0, bw), 0), (rng.uniform(0, bw), bh)][int(rng.integers(0, 4))]
    else:
        far = lambda n, k: float(n + rng.uniform(3, 9) + 8 / k) if rng.integers(0, 2) else float(-rng.uniform(3, 9) - 8 / k)
        u, v = (far(bw, min(kx, ky)), float(rng.uniform(-4, bh + 4))) if rng.integers(0, 2) else (float(rng.uniform(-4, bw + 4)), far(bh, min(kx, ky)))
    cx, cy = (x0 + w / 2) * 20 + float(rng.uniform(-10, 10)) * (aim != "outside"), (y0 + h / 2) * 20 + float(rng.uniform(-10, 10)) * (aim != "outside")
    a, b, cc, d = sx / 65536, r0 / 65536, r1 / 65536, sy / 65536          # x' = a u + cc v + tx, y' = b u + d v + ty  (twips)
    matrix = {"scale_x": sx, "scale_y": sy, "rotate_skew0": r0, "rotate_skew1": r1,
              "translate_x": int(round(cx - (a * u + cc * v))), "translate_y": int(round(cy - (b * u + d * v)))}
    fill = {"type": "bitmap", "bitmap_id": 7, "repeating": False, "smoothed": True, "pad": True, "matrix": matrix}
    scene = dict(width=FW, height=FH, exact=True, raw_bitmaps={7: (bw, bh, px.tobytes())}, stage={"children": [_shape(_box(x0, y0, x0 + w, y0 + h), fill)]})
    return dict(scene=scene, aim=aim, model=dict(matrices=[matrix], bitmap=px, rect=(x0, y0, x0 + w, y0 + h)))
