"""Gradient spread scenes ("Gradient spread modes") and their libcairo reference: FadeReplay -- so that "blend_mode",
"layer", "mask" and "opacity" mean what they mean in the other families -- over a backend that calls cairo_pattern_set_extend on every
gradient it creates, with the extend of the fill's "spread" (pad, reflect, repeat: swf-tree GradientSpread 0, 1, 2).

tools/make_spread_goldens.py writes goldens() to tests/golden/cairo_spread_*.npz (premultiplied RGBA; key = scene name); the tests
rebuild the scenes from here, so a golden file holds pixels only.  Frames are 200 x 45 (four tile columns, three tile-rows) and one
of 300 x 40.

Every gradient keeps its shape's rectangle within two radii of its centre, and the whole shape within two radii of its focus, on
both axes of the gradient square: cairo scales that square (+-16384) to +-16383 and pixman holds sample positions in 16.16.  A
rectangle that does not map into that range is not composited at all (pixman's analyze_extent), and a scanline's first position is
taken relative to the focus in 32 bits and wraps (the rest of the scanline is stepped in 64 bits): libcairo then paints nothing, or
something else.  Antialiased, a scanline starts at the rectangle's left edge; aliased, libcairo composites the shape box by box and a
scanline starts wherever a run of covered pixels does -- hence the whole shape.
tools/make_spread_goldens.py checks that: the padded rendering of every plain scene equals the oracle's.

The `runstart` files hold the exact boxes cut back to stepped polygons whose covered runs begin on a pixel where pixman's walker state
decides the colour (runstart_places finds them with tests/spread_model.py).  They stay out of files(), the list of what every device
route must reproduce byte for byte: there the device keeps its every-sample rule ("Gradient spread modes").

A non-pad LINEAR gradient is refused by the product (NotImplementedGradientSpread), so the non-pad scenes are radial and focal; one
padded linear scene rides along at LINEAR_BOUND.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import blend_scenes as bs  # noqa: E402
import fade_scenes as fs  # noqa: E402
import mask_scenes as ms  # noqa: E402
from scenarios import _m, _poly_shape, _rgba  # noqa: E402

LINEAR_BOUND = fs.LINEAR_BOUND
golden_path = bs.golden_path
W, H = 200, 45
SPREADS = ("reflect", "repeat")
CAIRO_EXTEND = {"pad": 3, "reflect": 2, "repeat": 1, 0: 3, 1: 2, 2: 1}       # cairo_extend_t of a spread's name or SWF number
R = 16384.0


def _backend(width, height):
    from oracle import cairo_backend as cb

    class SpreadBackend(cb.CairoBackend):
        """CairoBackend whose gradients get cairo_pattern_set_extend(self.extend) when they are created"""
        extend = CAIRO_EXTEND["pad"]

        def set_fill_radial(self, *a):
            super().set_fill_radial(*a)
            self.lib.cairo_pattern_set_extend(self._fill[1], self.extend)

        def set_fill_linear(self, *a):
            super().set_fill_linear(*a)
            self.lib.cairo_pattern_set_extend(self._fill[1], self.extend)
    return SpreadBackend(width, height)


class SpreadReplay(fs.FadeReplay):
    """FadeReplay that hands the spread of a path's gradient fill to the backend before the path is drawn"""

    def _draw_path(self, path):
        g = path.get("fill", {}).get("gradient")
        self.be.extend = CAIRO_EXTEND[(g or {}).get("spread", "pad")]
        return super()._draw_path(path)


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a spread scene through libcairo"""
    be = _backend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        low = ms._lowering(sc.get("bitmaps", []))
        stage = low.lower(sc["stage"])
        rp = SpreadReplay(be, linear_extension=True)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


def with_spread(obj, spread):
    """the same tree with every gradient's spread replaced"""
    if isinstance(obj, list):
        return [with_spread(o, spread) for o in obj]
    if isinstance(obj, dict):
        out = {k: with_spread(v, spread) for k, v in obj.items()}
        if "colors" in out and "spread" in out:
            out["spread"] = spread
        return out
    return obj


# ---- pieces
STOPS = {
    "ends": [(0, (255, 0, 0)), (90, (0, 255, 0)), (200, (20, 30, 120)), (255, (0, 0, 255))],          # stops at 0 and 255 and inner ones
    "inner": [(40, (255, 230, 0)), (128, (0, 90, 255)), (215, (250, 250, 250))],                     # no stop at either end
    "coincident": [(0, (255, 255, 255)), (102, (200, 0, 0)), (102, (0, 0, 200)), (255, (0, 40, 0))],  # a hard edge inside the ramp
    "single": [(77, (30, 200, 160))],
    "translucent": [(0, (255, 200, 0, 255)), (100, (0, 100, 255, 60)), (180, (255, 255, 255, 0)), (255, (255, 0, 255, 200))],
}


def _grad(stops, spread):
    return {"spread": spread, "color_space": "s-rgb", "colors": [{"ratio": t, "color": _rgba(*c)} for t, c in stops]}


def _fill(kind, matrix, stops, spread):
    f = {"type": {"radial": "radial-gradient", "linear": "linear-gradient"}.get(kind, "focal-gradient"), "matrix": matrix, "gradient": _grad(stops, spread)}
    if kind == "focal+":
        f["focal_point"] = {"epsilons": 192}
    elif kind == "focal-":
        f["focal_point"] = {"epsilons": -192}
    return f


def _quad(x0, y0, x1, y1):
    """a slanted quadrilateral (in pixels) inside the rectangle: antialiased edges all round"""
    return [(x0 + 1.3, y0 + 0.4), (x1 - 0.6, y0 + 1.7), (x1 - 2.2, y1 - 0.3), (x0 + 0.2, y1 - 1.6)]


def _shape(pts_px, fill, **kw):
    return {"type": "shape", "definition": _poly_shape([(round(x * 20), round(y * 20)) for x, y in pts_px], fill), **kw}


def _box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _scene(kids, w=W, h=H, exact=True):
    return dict(width=w, height=h, exact=exact, stage={"children": kids})


def _matrix(radius_px, cx, cy, sy=1.0, r0=0.0, r1=0.0):
    """the gradient square (+-16384) scaled to radius_px pixels around (cx, cy) pixels"""
    s = radius_px * 20 / R
    return _m(s, s * sy, round(cx * 20), round(cy * 20), r0 * s, r1 * s)


KINDS = ("radial", "focal+", "focal-")
KIND_PLACE = {"radial": (52, 100.3, 22.7), "focal-": (70, 113.7, 22.7), "focal+": (70, 86.3, 22.7)}       # radius and centre, in pixels
GROUND = [bs._shape([(3.3, 2.6), (W - 2.2, 4.1), (W - 5.4, H - 3.2), (1.7, H - 6.3)], (60, 140, 220, 150))]


def kind_scenes(spread):
    """every gradient kind x every stop list over a slanted quadrilateral that reaches into the second period on either side -- the
    even period 0 and the odd period 1; and the same over a translucent ground (OVER, not the first paint)"""
    out = {}
    for kind in KINDS:
        for sname, stops in STOPS.items():
            fill = _fill(kind, _matrix(*KIND_PLACE[kind]), stops, spread)
            out["%s_%s" % (kind.replace("+", "_pos").replace("-", "_neg"), sname)] = _scene([_shape(_quad(2, 1, 198, 44), fill)])
        fill = _fill(kind, _matrix(*KIND_PLACE[kind]), STOPS["translucent"], spread)
        out["%s_over_ground" % kind.replace("+", "_pos").replace("-", "_neg")] = _scene(GROUND + [_shape(_quad(2, 1, 198, 44), fill)])
    return out


# pixel-aligned boxes whose gradient centre sits on a pixel centre: samples fall exactly on stops and on period seams
# (a focal gradient whose focus lies to the right starts 1.2 radii left of the centre)
#   r32: radius 32 px, the pattern matrix is exact in 16.16, so along the centre's row the position is a whole multiple of 2048:
#        every 32nd pixel sits on a seam (and on the stops at 0 and 255)
#   r25: radius 25 px: positions n / 25 truncate onto the 16.16 stops at 51/255 and 102/255 (and, mirrored, 204/255)
EXACT = {
    "r32": (32, (40, 3, 160, 42), [(0, (255, 0, 0)), (128, (0, 255, 0, 128)), (255, (0, 0, 255))]),
    "r32_coincident": (32, (40, 3, 160, 42), [(0, (255, 255, 255)), (0, (0, 0, 0)), (255, (200, 0, 0)), (255, (0, 0, 200))]),
    "r25": (25, (52, 3, 148, 42), [(51, (255, 0, 0)), (102, (0, 255, 0)), (204, (0, 0, 255, 90))]),
    "r25_coincident": (25, (52, 3, 148, 42), [(0, (9, 9, 9)), (51, (255, 0, 0)), (51, (0, 255, 255)), (204, (0, 255, 0)), (204, (255, 0, 255)), (255, (0, 0, 90))]),
}


def exact_cases(spread):
    """name -> (scene, what tests/spread_model.py needs to paint it: swf matrices, circles, stops, the operation's rectangle)"""
    out = {}
    for name, (radius, rect, stops) in EXACT.items():
        for kind in KINDS:
            matrix = _matrix(radius, 100.5, 22.5)
            if kind == "focal+":
                rect = (100 - int(1.2 * radius) + 1,) + tuple(rect[1:])
            elif kind == "focal-":
                rect = tuple(rect[:2]) + (101 + int(1.2 * radius), rect[3])
            fill = _fill(kind, matrix, stops, spread)
            focal = {"radial": 0.0, "focal+": 0.75, "focal-": -0.75}[kind]
            model = dict(matrices=[matrix], circles=(focal * R, 0.0, 0.0, 0.0, 0.0, R), rect=rect,
                         stops=[(t / 255, c[0] / 255, c[1] / 255, c[2] / 255, (c[3] if len(c) > 3 else 255) / 255) for t, c in stops])
            out["%s_%s" % (kind.replace("+", "_pos").replace("-", "_neg"), name)] = (_scene([_shape(_box(*rect), fill)]), model)
    return out


def exact_scenes(spread):
    return {name: sc for name, (sc, _) in exact_cases(spread).items()}


def structure_scenes(spread):
    """a rotated and skewed gradient matrix, a squeezed one, a colour transform around, and one scene each under "blend_mode", "layer",
    "mask" and "opacity"; a padded gradient beside a spread one in one frame; the padded linear extension"""
    import make_cxform_goldens as mk
    out = {}
    stops = STOPS["ends"]
    shape = lambda fill, box=(2, 1, 198, 44), **kw: _shape(_quad(*box), fill, **kw)
    out["rotated_skewed"] = _scene([shape(_fill("radial", _matrix(60, 101.2, 21.4, 0.7, 0.45, -0.3), stops, spread))])
    out["focal_rotated"] = _scene([shape(_fill("focal+", _matrix(70, 80.1, 23.3, 0.8, -0.5, 0.5), STOPS["inner"], spread))])
    out["object_matrix"] = _scene([shape(_fill("radial", _matrix(54, 100.3, 22.7), STOPS["coincident"], spread), matrix=_m(0.9, 0.95, 180, 20, 0.02, -0.03))])
    tint = mk.cxform(mult=(256, 200, 128, 160), add=(0, 20, 60, 0))
    out["cxform_around"] = _scene(GROUND + [{"type": "container", "color_transform": tint, "children": [shape(_fill("radial", _matrix(54, 100.3, 22.7), stops, spread))]}])
    grad = shape(_fill("focal-", _matrix(*KIND_PLACE["focal-"]), STOPS["translucent"], spread))
    out["blend_mode"] = _scene(GROUND + [dict(grad, blend_mode="multiply")])
    out["layer"] = _scene(GROUND + [{"type": "container", "layer": "screen", "children": [grad, bs._rect(60, 8, 120, 30, (200, 20, 20, 100))]}])
    out["mask"] = _scene(GROUND + [{"type": "container", "children": [bs._rect(10, 4, 190, 40, (20, 200, 90, 230))], "mask": [grad]}])
    out["opacity"] = _scene(GROUND + [{"type": "container", "opacity": 150, "children": [grad, bs._rect(60, 8, 120, 30, (200, 20, 20, 100))]}])
    # a padded and a spread gradient in one frame: both walkers in one launch, per style
    out["beside_pad"] = _scene([shape(_fill("radial", _matrix(30, 50.5, 22.2), stops, "pad"), (2, 1, 98, 44)),
                                shape(_fill("radial", _matrix(30, 150.5, 22.2), stops, spread), (102, 1, 198, 44))])
    out["linear_pad"] = _scene([shape(_fill("linear", _matrix(54, 100.3, 22.7), stops, "pad"))], exact=False)
    return out


def wide_scenes(spread):
    """300 x 40: the frame of the two-band routes (five tile columns, three tile-rows)"""
    return {"wide": _scene([_shape(_quad(3, 1, 297, 39), _fill("radial", _matrix(80, 150.4, 19.6), STOPS["translucent"], spread))], 300, 40)}


def _kinds_of(prefix):
    return lambda spread: {n: s for n, s in kind_scenes(spread).items() if n.startswith(prefix)}


# ---- covered runs that begin on a sample where the walker's state decides ("Gradient spread modes": the caveat)
def _stepped(rect, x, gap):
    """the rectangle's first row whole, the rows below from column x on -- and, with a gap, a block at the rectangle's left edge too, so
    that the run at x is the second of its row.  Whole pixels; the pixel extents stay the rectangle's."""
    x0, y0, x1, y1 = rect
    if not gap:
        return [(x0, y0), (x1, y0), (x1, y1), (x, y1), (x, y0 + 1), (x0, y0 + 1)]
    xg = x0 + (x - x0) // 2
    return [(x0, y0), (x1, y0), (x1, y1), (x, y1), (x, y0 + 1), (xg, y0 + 1), (xg, y1), (x0, y1)]


def runstart_places():
    """[(exact case, column, the rows where a fresh reset paints otherwise there)] -- found by tests/spread_model.py in the REFLECT
    exact cases, not written down: every column that holds a pixel where the stateful walker and a fresh reset disagree"""
    import numpy as np
    import spread_model as sm
    out = []
    for name, (_, md) in sorted(exact_cases("reflect").items()):
        x0, y0, x1, y1 = md["rect"]
        src = sm.source(sm.pattern_matrix(md["matrices"]), md["circles"], md["stops"], sm.REFLECT, md["rect"])
        ys, xs = np.nonzero(src["stateful"] != src["fresh"])
        for x in sorted(set(int(v) for v in xs)):
            rows = [int(y) + y0 for y in ys[xs == x]]
            if x > 0 and min(rows) > y0:         # (a run cannot begin left of the rectangle; the first row stays whole)
                out.append((name, x + x0, rows))
    return out


def runstart_cases(spread, aliased=False):
    """name -> a tests/spread_fuzz.py case: the exact case's box cut back to a stepped polygon whose covered runs begin in the column
    of a state pixel; for the last place also with a block left of a gap in the same rows, that once more off the pixel grid, and as a box that begins in the column
    (`edge`: no sample lies to the left inside the rectangle, so there the every-sample rule is libcairo's).  The same outlines under
    either spread: REPEAT has no such pixel, and must show none.  `caveat`: whether REFLECT shows caveat pixels there (`rows`, `column`)."""
    import spread_fuzz as sf
    out = {}
    places = runstart_places()
    for k, (name, x, rows) in enumerate(places):
        kind = [kd for kd in KINDS if name.startswith(kd.replace("+", "_pos").replace("-", "_neg"))][0]
        radius, _, stops = EXACT["r" + name.split("_r", 1)[1]]
        rect = exact_cases(spread)[name][1]["rect"]
        stops = [(t, tuple(c) + (255,) * (4 - len(c))) for t, c in stops]
        eps = {"radial": 0, "focal+": 192, "focal-": -192}[kind]
        make = lambda pts, **kw: sf.make_case(W, H, aliased, spread, kind, _matrix(radius, 100.5, 22.5), eps, stops, pts, "runstart", column=x, rows=rows, **kw)
        for gap in ((False, True) if k == len(places) - 1 else (False,)):
            key = "%s_x%d%s" % (name, x, "_gap" if gap else "")
            out[key] = make(_stepped(rect, x, gap), edge=False, caveat=True)
            assert out[key]["model"]["rect"] == tuple(rect)
        if k == len(places) - 1:                 # the gap once more with one corner off the grid: antialiased, libcairo then composites through
            pts = _stepped(rect, x, True)        # a mask and ONE walker crosses the gap, skipping its samples
            out["%s_x%d_mask" % (name, x)] = make(pts[:-1] + [(pts[-1][0], pts[-1][1] - 0.5)], edge=False, caveat=bool(aliased))
        if k == len(places) - 1:                 # the rectangle itself begins in the column: every walker starts there, the device's too
            out["%s_x%d_edge" % (name, x)] = make(_box(x, rect[1], rect[2], rect[3]), edge=True, caveat=False)
    return out


def runstart_scenes(spread):
    return {name: case["scene"] for name, case in runstart_cases(spread).items()}


GROUPS = {"radial": _kinds_of("radial"), "focal_pos": _kinds_of("focal_pos"), "focal_neg": _kinds_of("focal_neg"), "exact": exact_scenes,
          "structure": lambda spread: dict(structure_scenes(spread), **wide_scenes(spread))}


def all_scenes(spread):
    out = {}
    for make in GROUPS.values():
        out.update(make(spread))
    return out


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        for spread in SPREADS:
            for group, make in GROUPS.items():
                out["cairo_spread_%s%s_%s" % ("aliased_" if aliased else "", spread, group)] = ((lambda s=spread, m=make: m(s)), aliased)
    return out


def runstart_files():
    """the same for the run-start scenes.  They are NOT in files(): the device paints them by its every-sample rule, a whole colour
    away from libcairo in the caveat pixels of spread_model.frame (tests/test_spread_fuzz_gpu.py pins both)"""
    return {"cairo_spread_%s%s_runstart" % ("aliased_" if aliased else "", spread): ((lambda s=spread: runstart_scenes(s)), aliased)
            for aliased in (False, True) for spread in SPREADS}


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())}
            for fname, (make, aliased) in dict(files(), **runstart_files()).items()}
