"""Pixman-exact linear gradient scenes ("Pixman-exact linear gradients") and their libcairo reference: the spread family's
replay (tests/spread_scenes.py: SpreadReplay sets cairo_pattern_set_extend from the fill's "spread"), so "blend_mode", "layer", "mask"
and "opacity" mean what they mean in the other families.

tools/make_linear_goldens.py writes goldens() to tests/golden/cairo_linear_*.npz (premultiplied RGBA; key = scene name); the tests
rebuild the scenes from here, so a golden file holds pixels only.  Frames are 130 x 40 -- three tile columns, three tile-rows, the
shape's rectangle starting at column 5: the smallest shape at which a strip boundary, the origin of a row's piece and the row step can
each go wrong -- two of 600 x 20, whose rows libcairo cuts into several pieces, and the `gradient_linear_ext` fill of
tests/scenarios.py at its own 130 x 115.

The product renders these only on a handle created with linear="pixman" (SWFR_FLAG_LINEAR_PIXMAN); a default handle refuses the
reflected and repeated ones as before.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_scenes as bs  # noqa: E402
import spread_scenes as ss  # noqa: E402
from scenarios import _m, scenarios  # noqa: E402

LINEAR_BOUND = 0                                 # (device_routes.check reads it for a scene that is not exact: there is none here)
golden_path = bs.golden_path
cairo_render = ss.cairo_render
W, H = 130, 40
SPREADS = ("pad", "reflect", "repeat")
R = ss.R
STOPS = ss.STOPS


def matrix(kind, half_px=24.0, cx=66.3, cy=19.7):
    """the gradient line (-16384, 0)-(16384, 0) scaled to 2 * half_px pixels around (cx, cy) pixels: horizontal, vertical (turned by a
    right angle: every row is one colour), rotated, sheared"""
    s = half_px * 20 / R
    tx, ty = round(cx * 20), round(cy * 20)
    if kind == "horizontal":
        return _m(s, s, tx, ty)
    if kind == "vertical":
        return _m(0.0, 0.0, tx, ty, 0.4 * s, -2.0 * s)
    if kind == "rotated":
        return _m(0.8 * s, 0.8 * s, tx, ty, 0.6 * s, -0.6 * s)
    assert kind == "sheared"
    return _m(s, 0.7 * s, tx, ty, 0.0, 0.55 * s)


MATRICES = ("horizontal", "vertical", "rotated", "sheared")


def fill(kind, stops, spread, **kw):
    return ss._fill("linear", matrix(kind, **kw), stops, spread)


def plain_scenes(spread):
    """every matrix under a slanted quadrilateral (composited row by row through the span renderer) and under one box on whole
    pixels; a shape the frame's left edge cuts; coincident and translucent stops; a concave shape (rows with two covered runs); a box
    off the pixel grid; the gradient_linear_ext fill of the scenarios"""
    out = {}
    for kind in MATRICES:
        out["poly_" + kind] = ss._scene([ss._shape(ss._quad(5, 1, 128, 39), fill(kind, STOPS["ends"], spread))], W, H)
        out["box_" + kind] = ss._scene([ss._shape(ss._box(5, 2, 127, 38), fill(kind, STOPS["inner"], spread))], W, H)
    out["cut_left"] = ss._scene([ss._shape([(-9.3, 3.2), (90.4, 1.7), (120.6, 37.1), (-4.2, 38.6)], fill("rotated", STOPS["ends"], spread))], W, H)
    out["coincident"] = ss._scene([ss._shape(ss._quad(5, 1, 128, 39), fill("sheared", STOPS["coincident"], spread))], W, H)
    out["translucent"] = ss._scene(ss.GROUND[:0] + [bs._shape([(3.3, 2.6), (W - 2.2, 4.1), (W - 5.4, H - 3.2), (1.7, H - 6.3)], (60, 140, 220, 150)),
                                                  ss._shape(ss._quad(5, 1, 128, 39), fill("rotated", STOPS["translucent"], spread))], W, H)
    notch = [(5.4, 1.3), (50.2, 2.1), (66.7, 30.4), (80.3, 1.6), (127.2, 2.8), (125.1, 38.2), (6.6, 37.4)]
    out["notched"] = ss._scene([ss._shape(notch, fill("horizontal", STOPS["ends"], spread, half_px=17.0))], W, H)
    out["box_off_grid"] = ss._scene([ss._shape(ss._box(5.35, 2.4, 126.7, 37.55), fill("rotated", STOPS["inner"], spread))], W, H)
    # boxes on whole pixels under a MIRRORED horizontal matrix of 50 pixels a gradient length, centred on a pixel centre: positions fall
    # along the row and samples sit exactly on coincident stops; under reflect, in an odd period, the walker's state decides those
    # pixels (two a row with the first stop list, in columns other than the rectangle's first: tests/test_linear_model.py counts them)
    for key in ("r25_coincident", "r32_coincident"):
        s = 25.0 * 20 / R
        out["box_exact_" + key] = ss._scene([ss._shape(ss._box(5, 2, 127, 38), ss._fill("linear", _m(-s, s, 810, 400), ss.EXACT[key][2], spread))], W, H)
    # 600 x 20: rows with runs of 256 and more full pixels, which libcairo composites as pieces of their own, and (the notch) an empty
    # span behind more than 256 gathered pixels
    wide = dict(half_px=120.0, cx=301.3, cy=9.6)
    out["wide_runs"] = ss._scene([ss._shape(ss._quad(5, 1, 597, 19), fill("horizontal", STOPS["ends"], spread, **wide))], 600, 20)
    wnotch = [(5.4, 1.3), (300.2, 2.1), (340.7, 16.4), (380.3, 1.6), (596.2, 2.8), (594.1, 18.2), (6.6, 17.4)]
    out["wide_notched"] = ss._scene([ss._shape(wnotch, fill("rotated", STOPS["inner"], spread, **wide))], 600, 20)
    ext = scenarios()["gradient_linear_ext"]
    out["config_fill"] = ss.with_spread(dict(width=ext["width"], height=ext["height"], exact=True, stage=ext["stage"]), spread)
    return out


def structure_scenes(spread):
    """one scene each under a colour transform, a blend mode, a layer, a masked layer and a faded layer"""
    import make_cxform_goldens as mk
    out = {}
    ground = [bs._shape([(3.3, 2.6), (W - 2.2, 4.1), (W - 5.4, H - 3.2), (1.7, H - 6.3)], (60, 140, 220, 150))]
    grad = ss._shape(ss._quad(5, 1, 128, 39), fill("rotated", STOPS["translucent"], spread))
    tint = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
    out["cxform_around"] = ss._scene(ground + [{"type": "container", "color_transform": tint, "children": [ss._shape(ss._quad(5, 1, 128, 39), fill("sheared", STOPS["ends"], spread))]}], W, H)
    out["blend_mode"] = ss._scene(ground + [dict(grad, blend_mode="multiply")], W, H)
    out["layer"] = ss._scene(ground + [{"type": "container", "layer": "screen", "children": [grad, bs._rect(40, 8, 90, 30, (200, 20, 20, 100))]}], W, H)
    out["mask"] = ss._scene(ground + [{"type": "container", "children": [bs._rect(10, 4, 120, 36, (20, 200, 90, 230))], "mask": [grad]}], W, H)
    out["opacity"] = ss._scene(ground + [{"type": "container", "opacity": 150, "children": [grad, bs._rect(40, 8, 90, 30, (200, 20, 20, 100))]}], W, H)
    return out


GROUPS = {"plain": plain_scenes, "structure": structure_scenes}


def all_scenes(spread):
    out = {}
    for make in GROUPS.values():
        out.update(make(spread))
    return out


def files():
    """golden file name -> (scenes, aliased): antialiased only -- aliased, a pixman-linear gradient is refused"""
    return {"cairo_linear_%s_%s" % (spread, group): ((lambda s=spread, m=make: m(s)), False) for spread in SPREADS for group, make in GROUPS.items()}


def goldens():
    return {fname: {name: cairo_render(sc) for name, sc in sorted(make().items())} for fname, (make, _) in files().items()}
