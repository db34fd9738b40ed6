"""Pins oracle/swfr_oracle.c against the container's libcairo 1.16.0 by fuzzing (skipped where the
library is absent; the committed goldens cover the same ground on the GPU box)."""
import zlib

import numpy as np
import pytest

from helpers import LARGE_MODES, LIMIT, large_pts
from oracle import cairo_backend as cb, oracle_backend as ob

pytestmark = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")


def _draw(be, ops):
    be.set_transform_identity()
    be.clear_all()
    for op in ops:
        if op[0] == "poly":
            _, pts, col, eo, curves = op
            be.begin_path()
            be.move_to(*pts[0])
            i = 1
            while i < len(pts):
                if curves and i + 1 < len(pts) and curves[i]:
                    be.quadratic_curve_to(pts[i][0], pts[i][1], pts[i + 1][0], pts[i + 1][1])
                    i += 2
                else:
                    be.line_to(*pts[i])
                    i += 1
            be.set_fill_rule(eo)
            be.set_fill_rgba(*col)
            be.fill()
        elif op[0] == "stroke":
            _, pts, col, wd = op
            be.begin_path()
            be.move_to(*pts[0])
            for p in pts[1:]:
                be.line_to(*p)
            be.set_line_width(wd)
            be.set_stroke_rgba(*col)
            be.stroke()
        else:                                  # "pen": strokes with every style knob (dict)
            o = op[1]
            if o.get("matrix"):
                be.transform(*o["matrix"])
            if o.get("scale"):
                be.scale(*o["scale"])
            be.begin_path()
            for sub in o["subs"]:
                pts, curves, closed = sub
                be.move_to(*pts[0])
                i = 1
                while i < len(pts):
                    if curves and i + 1 < len(pts) and curves[i]:
                        be.quadratic_curve_to(pts[i][0], pts[i][1], pts[i + 1][0], pts[i + 1][1])
                        i += 2
                    else:
                        be.line_to(*pts[i])
                        i += 1
                if closed:
                    be.close_path()
            be.set_line_width(o["w"])
            be.set_line_cap(o["cap"])
            be.set_line_join(o["join"])
            be.set_stroke_rgba(*o["col"])
            be.stroke()


def _same(W, H, ops):
    a = cb.CairoBackend(W, H); _draw(a, ops); ca = a.premultiplied_rgba(); a.close()
    b = ob.OracleBackend(W, H); _draw(b, ops); oa = b.premultiplied_rgba(); b.close()
    return (ca == oa).all()


def _pts(rng, W, H, n, mode):
    if mode == "quarter":
        return [(float(rng.integers(0, 4 * W)) / 4, float(rng.integers(0, 4 * H)) / 4) for _ in range(n)]
    if mode == "integer":
        return [(float(rng.integers(0, W)), float(rng.integers(0, H))) for _ in range(n)]
    if mode == "offframe":
        return [(float(rng.uniform(-30, W + 30)), float(rng.uniform(-30, H + 30))) for _ in range(n)]
    if mode == "shallow":
        y = rng.uniform(0, H)
        return [(float(rng.uniform(0, W)), float(y + rng.uniform(-2, 2))) for _ in range(n)]
    if mode == "steep":
        x = rng.uniform(0, W)
        return [(float(x + rng.uniform(-2, 2)), float(rng.uniform(0, H))) for _ in range(n)]
    if mode in LARGE_MODES:
        return large_pts(rng, W, H, n, mode)
    return [(float(rng.uniform(0, W)), float(rng.uniform(0, H))) for _ in range(n)]


@pytest.mark.parametrize("mode", ["uniform", "quarter", "integer", "offframe", "shallow", "steep"] + list(LARGE_MODES))
def test_polygons_both_fill_rules(mode):
    rng = np.random.default_rng(zlib.crc32(mode.encode()) % 1000)
    for _ in range(250):
        W, H = int(rng.integers(16, 64)), int(rng.integers(16, 64))
        ops = [("poly", _pts(rng, W, H, int(rng.integers(3, 9)), mode), (int(rng.integers(0, 256)), 7, 99, 255),
                bool(rng.integers(0, 2)), None)]
        assert _same(W, H, ops), ops


def test_quadratic_curves():
    rng = np.random.default_rng(3)
    for _ in range(250):
        n = int(rng.integers(4, 9))
        ops = [("poly", _pts(rng, 48, 40, n, "uniform"), (10, 200, 30, 255), False, [bool(rng.integers(0, 2)) for _ in range(n)])]
        assert _same(48, 40, ops), ops


@pytest.mark.parametrize("mode", LARGE_MODES)
def test_quadratic_curves_at_large_magnitudes(mode):
    """Curves whose control and end points lie up to 32768 px away: flattening with long chords, clipped to the frame."""
    rng = np.random.default_rng(zlib.crc32(("curves" + mode).encode()) % 1000)
    painted = 0
    for _ in range(150):
        n = int(rng.integers(4, 9))
        ops = [("poly", _pts(rng, 48, 40, n, mode), (10, 200, 30, int(rng.choice([255, 130]))), bool(rng.integers(0, 2)),
                [bool(rng.integers(0, 2)) for _ in range(n)])]
        a = cb.CairoBackend(48, 40); _draw(a, ops); ca = a.premultiplied_rgba(); a.close()
        b = ob.OracleBackend(48, 40); _draw(b, ops); oa = b.premultiplied_rgba(); b.close()
        assert (ca == oa).all(), ops
        painted += int(((ca[..., 3] > 0) & (ca[..., 3] < 255)).sum())
    assert painted > 500          # edges do cross the frame (partial coverage), not only empty or full frames


def test_translucent_painters_order():
    rng = np.random.default_rng(4)
    for _ in range(250):
        ops = [("poly", _pts(rng, 40, 40, int(rng.integers(3, 7)), "uniform"),
                (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.choice([255, 128, 37, 200, 1, 254]))),
                False, None) for _ in range(3)]
        assert _same(40, 40, ops), ops


def test_open_strokes_miter_butt():
    rng = np.random.default_rng(5)
    for _ in range(400):
        ops = [("stroke", _pts(rng, 48, 40, int(rng.integers(2, 7)), "uniform"), (0, 0, 0, 255), float(rng.uniform(0.5, 6)))]
        assert _same(48, 40, ops), ops


def test_rectangles_box_path():
    rng = np.random.default_rng(6)
    for _ in range(250):
        ops = []
        for _k in range(int(rng.integers(1, 4))):
            x0, y0 = rng.uniform(-5, 40), rng.uniform(-5, 40)
            x1, y1 = x0 + rng.uniform(0, 30), y0 + rng.uniform(0, 30)
            q = lambda v: float(np.round(v * rng.choice([1, 2, 4, 20])) / rng.choice([1, 2, 4, 20]))
            x0, y0, x1, y1 = map(q, (x0, y0, x1, y1))
            ops.append(("poly", [(x0, y0), (x1, y0), (x1, y1), (x0, y1)], (int(rng.integers(0, 256)), 9, 0, int(rng.choice([255, 100]))), False, None))
        assert _same(40, 40, ops), ops


# ---- the full stroker (cairo-path-stroke-polygon.c + pen + rectilinear box stroker): caps, joins, closed sub-paths, curves
def _pen_case(rng, W, H, *, cap=None, join=None, closed=None, curves=False, rect=False, wmin=0.3, wmax=8.0, margin=0, scale=False, subs=1):
    out = []
    for _ in range(subs):
        n = int(rng.integers(2, 7))
        if rect:
            x, y = float(rng.integers(-4, W - 4)), float(rng.integers(-4, H - 4))
            pts = [(x, y)]
            for k in range(n):
                if k % 2 == 0:
                    x = float(rng.integers(-6, W + 2)) + float(rng.choice([0, 0.5, 0.25]))
                else:
                    y = float(rng.integers(-6, H + 4)) + float(rng.choice([0, 0.5, 0.25]))
                pts.append((x, y))
        else:
            pts = [(float(rng.uniform(margin, W - margin)), float(rng.uniform(margin, H - margin))) for _ in range(n)]
        cv = [bool(rng.integers(0, 3) == 0) for _ in range(len(pts))] if curves else None
        out.append((pts, cv, bool(rng.integers(0, 2)) if closed is None else closed))
    return ("pen", dict(subs=out, w=float(rng.uniform(wmin, wmax)),
                        cap=int(rng.integers(0, 3)) if cap is None else cap,
                        join=int(rng.integers(0, 3)) if join is None else join,
                        col=(int(rng.integers(0, 256)), 20, 30, int(rng.choice([255, 255, 120]))),
                        scale=(float(rng.choice([-1, 1]) * rng.uniform(0.5, 2)), float(rng.uniform(0.5, 2))) if scale and rng.integers(0, 2) else None))


def _large_scale(rng, op, W, H):
    """Places a pen case under a uniform stage scale up to the point where the path reaches +-32768 px (the limit of the product's
    device range), translated so that some part of the stroke stays near the frame."""
    o = op[1]
    xs = [p[0] for sub in o["subs"] for p in sub[0]]
    ys = [p[1] for sub in o["subs"] for p in sub[0]]
    reach = max(max(map(abs, xs)), max(map(abs, ys)), 1.0)
    k = float(rng.uniform(0.5, 1.0)) * (LIMIT - 2 * max(W, H)) / reach / (2 if rng.integers(0, 2) else 1)
    cx, cy = xs[0], ys[0]                     # the first vertex lands inside the frame
    # (a reflection or a non-uniform scale only without round joins and caps: see test_round_join_under_a_non_uniform_scale_known_difference)
    round_pen = o["join"] == 1 or o["cap"] == 1
    ky = k * float(rng.choice([1, -1, 0.5])) if not round_pen else k
    o["matrix"] = (k, 0.0, 0.0, ky, float(rng.uniform(0, W)) - k * cx, float(rng.uniform(0, H)) - ky * cy)
    o["scale"] = None
    # 0.5 to 40 device pixels wide, or up to several thousand
    o["w"] = float(rng.uniform(0.5, 40.0)) / k if rng.integers(0, 3) else float(rng.uniform(0.02, 4.0))
    return op


@pytest.mark.parametrize("kind", ["round_join", "bevel_join", "round_cap", "square_cap", "closed", "curves", "rectilinear", "hairline", "everything",
                                  "large_scale", "large_scale_rectilinear"])
def test_stroker_styles(kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) % 997)
    W, H = 48, 40
    varied = 0
    for _ in range(250):
        if kind == "large_scale":
            op = _large_scale(rng, _pen_case(rng, W, H, curves=True, margin=-12, subs=int(rng.integers(1, 3))), W, H)
        elif kind == "large_scale_rectilinear":
            op = _large_scale(rng, _pen_case(rng, W, H, rect=True, join=int(rng.choice([0, 0, 1, 2])), cap=int(rng.choice([0, 2]))), W, H)
        elif kind == "round_join":
            op = _pen_case(rng, W, H, cap=0, join=1, closed=False)
        elif kind == "bevel_join":
            op = _pen_case(rng, W, H, cap=0, join=2, closed=False)
        elif kind == "round_cap":
            op = _pen_case(rng, W, H, cap=1, join=0, closed=False)
        elif kind == "square_cap":
            op = _pen_case(rng, W, H, cap=2, join=0, closed=False)
        elif kind == "closed":
            op = _pen_case(rng, W, H, closed=True, margin=5)
        elif kind == "curves":
            op = _pen_case(rng, W, H, curves=True, margin=3)
        elif kind == "rectilinear":
            op = _pen_case(rng, W, H, rect=True, join=int(rng.choice([0, 0, 0, 1, 2])), wmin=0.02, wmax=4.0, scale=True)
        elif kind == "hairline":        # line width <= tolerance / 2 under the CTM: cairo draws nothing
            op = _pen_case(rng, W, H, wmin=0.005, wmax=0.3, scale=True)
        else:
            op = _pen_case(rng, W, H, curves=True, margin=-12, scale=True, subs=int(rng.integers(1, 4)))
        assert _same(W, H, [op]), op
        if kind.startswith("large_scale"):
            a = cb.CairoBackend(W, H); _draw(a, [op]); img = a.premultiplied_rgba()[..., 3]; a.close()
            varied += bool((img != img.flat[0]).any())
    if kind.startswith("large_scale"):
        assert varied > 150           # most frames show an outline's edge, not only an empty or uniformly covered frame


@pytest.mark.xfail(strict=True, reason="known oracle difference: one pixel of a round join under a non-uniform scale, 2/255 off")
def test_round_join_under_a_non_uniform_scale_known_difference():
    """Found by the large-scale stroke fuzz, but independent of the magnitudes (the same device geometry drawn from user coordinates
    near the origin differs the same way; a uniform scale or a 3 px shift does not): a closed four-point path with round joins,
    a pen 33 x 16 device pixels wide.  One pixel of the oracle is 181 where libcairo gives 179.  Pinned here so that a fix of the
    oracle's pen / fan restatement shows up.  Reflected large pens (y scale -k) differ in the same way; the large-scale fuzz keeps
    reflections and non-uniform scales to miter and bevel joins until then."""
    op = ("pen", dict(subs=[([(56.256924568088294, 10.381050109408882), (6.631615315619026, 8.70962727024363),
                              (31.900229039925122, 39.502684441614086), (33.37925896304273, 39.51596599539821)], None, True)],
                      w=0.17924089612921035, cap=0, join=1, col=(103, 20, 30, 255), scale=None,
                      matrix=(184.16369457889198, 0.0, 0.0, 92.08184728944599, -10333.66549487574, -940.9449840521969)))
    assert _same(48, 40, [op])


# ---- bitmap fills: CAIRO_FILTER_GOOD = bilinear above scale 0.75, pixman's separable convolution below.  Tables and accumulation
#      are pixman's integers; the sample position comes from the double matrix (pixman rounds its matrix to 16.16 first), so a small
#      share of the pixels may sit an LSB or two off.  EXTEND_REPEAT keeps the bitmap's own border out of the picture.
@pytest.mark.parametrize("repeat", [True, False])
@pytest.mark.parametrize("kind", ["minify_rotated", "minify_axis", "mixed", "magnify"])
def test_bitmap_fill_filters(kind, repeat):
    """Surface patterns under CAIRO_FILTER_GOOD, both extend modes: bilinear / separable convolution at pixman's 16.16 sample
    positions (matrix rounded and re-centred on the operation's rectangle), EXTEND_NONE bounded by the source extents: bit-exact."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()) % 991)
    W, H = 64, 48
    for _ in range(40):
        tw, th = int(rng.integers(8, 40)), int(rng.integers(8, 40))
        bmp = rng.integers(0, 256, (th, tw, 4)).astype(np.uint8)
        if rng.integers(0, 2):
            bmp[..., 3] = 255
        lo, hi, rot = {"minify_rotated": (0.1, 0.7, True), "minify_axis": (0.05, 0.74, False), "mixed": (0.3, 3.0, True), "magnify": (0.76, 6.0, True)}[kind]
        sx, sy = rng.uniform(lo, hi), rng.uniform(lo, hi)
        th_ = rng.uniform(-0.6, 0.6) if rot else 0.0
        c, s_ = np.cos(th_), np.sin(th_)
        m = (sx * c, sx * s_, -sy * s_, sy * c, float(rng.uniform(-5, 20)), float(rng.uniform(-5, 20)))
        imgs = []
        for be in (cb.CairoBackend(W, H), ob.OracleBackend(W, H)):
            be.set_transform_identity(); be.clear_all()
            b = be.create_bitmap(tw, th, bmp.tobytes())
            be.begin_path(); be.move_to(2, 2); be.line_to(W - 3, 3); be.line_to(W - 2, H - 2); be.line_to(3, H - 4); be.line_to(2, 2)
            be.save(); be.transform(*m)
            be.set_fill_pattern(b, repeat); be.fill(); be.restore()
            imgs.append(be.premultiplied_rgba().astype(int)); be.close()
        assert np.array_equal(imgs[0], imgs[1]), (kind, repeat, m, tw, th)


@pytest.mark.parametrize("seed", list(range(1, 11)))
def test_bitmap_fill_scenes(seed):
    """Whole drawing sequences as the renderer issues them (scale(1/20); optional object matrix; per fill save / transform(fill
    matrix) / fill / restore): one to three overlapping bitmap fills per frame -- polygons, curves, unaligned and pixel-aligned
    rectangles, off-frame geometry, reflections, 1x1 to 40x40 bitmaps from 20x minified to 40x magnified, repeat and no-repeat,
    on a clear surface and on top of each other.  Bit-exact."""
    rng = np.random.default_rng(seed)
    painted = 0
    for it in range(50):
        W, H = int(rng.integers(20, 90)), int(rng.integers(20, 70))
        tw, th = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        bmp = rng.integers(0, 256, (th, tw, 4)).astype(np.uint8)
        if rng.integers(0, 2):
            bmp[..., 3] = 255
        ops = []
        for k in range(int(rng.integers(1, 4))):
            lo, hi = [(0.05, 0.74), (0.3, 3.0), (0.76, 8.0), (15, 40)][int(rng.integers(0, 4))]
            sx, sy = rng.uniform(lo, hi), rng.uniform(lo, hi)
            t = rng.uniform(-3.2, 3.2) if rng.integers(0, 3) else 0.0
            c, s_ = np.cos(t), np.sin(t)
            if rng.integers(0, 5) == 0:
                sx = -sx
            fm = (sx * c * 20, sx * s_ * 20, -sy * s_ * 20, sy * c * 20, float(rng.integers(-200, 1500)), float(rng.integers(-200, 1200)))
            kind = int(rng.integers(0, 4))
            if kind == 0:     # polygon in twips, partly off-frame
                pts = [(int(rng.integers(-300, W * 20 + 300)), int(rng.integers(-300, H * 20 + 300))) for _ in range(int(rng.integers(3, 7)))]
            elif kind == 1:   # rectangle, not pixel aligned
                x0, y0 = int(rng.integers(-100, W * 10)), int(rng.integers(-100, H * 10))
                x1, y1 = x0 + int(rng.integers(50, W * 15)), y0 + int(rng.integers(50, H * 15))
                pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
            elif kind == 2:   # rectangle, pixel aligned
                x0, y0 = 20 * int(rng.integers(0, W // 2)), 20 * int(rng.integers(0, H // 2))
                x1, y1 = x0 + 20 * int(rng.integers(1, W)), y0 + 20 * int(rng.integers(1, H))
                pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
            else:             # one curved side
                pts = [(int(rng.integers(0, W * 20)), int(rng.integers(0, H * 20))) for _ in range(4)]
            ops.append((fm, pts, bool(rng.integers(0, 2)), kind == 3))
        om = (float(rng.uniform(0.5, 2.0)), 0.0, 0.0, float(rng.uniform(0.5, 2.0)), float(rng.integers(-100, 100)), float(rng.integers(-100, 100))) if rng.integers(0, 2) else None
        imgs = []
        for be in (cb.CairoBackend(W, H), ob.OracleBackend(W, H)):
            be.set_transform_identity(); be.clear_all(); be.scale(1 / 20, 1 / 20)
            b = be.create_bitmap(tw, th, bmp.tobytes())
            be.save()
            if om:
                be.transform(*om)
            for fm, pts, rep, curved in ops:
                be.begin_path(); be.move_to(*pts[0])
                if curved:
                    be.quadratic_curve_to(pts[1][0], pts[1][1], pts[2][0], pts[2][1]); be.line_to(*pts[3])
                else:
                    for q in pts[1:]:
                        be.line_to(*q)
                be.line_to(*pts[0])
                be.save(); be.transform(*fm)
                be.set_fill_pattern(b, rep); be.fill(); be.restore()
            be.restore()
            imgs.append(be.premultiplied_rgba().astype(int)); be.close()
        assert np.array_equal(imgs[0], imgs[1]), (seed, it)
        painted += int((imgs[0][..., 3] > 0).sum())
    assert painted > 8000


@pytest.mark.parametrize("seed", [7, 8, 9, 10])
def test_bitmap_scenes_through_the_canvas_replay(seed):
    """The scenes of the GPU bitmap fuzz (tests/helpers.py rand_bitmap_scene: swf-tree shapes with bitmap fills, drawn by the
    restated CanvasRenderer) rendered by libcairo and by the oracle: identical frames."""
    from helpers import rand_bitmap_scene
    from oracle import canvas_replay as cr
    rng = np.random.default_rng(seed)
    for it in range(40):
        sc = rand_bitmap_scene(rng)
        imgs = []
        for be in (cb.CairoBackend(sc["width"], sc["height"]), ob.OracleBackend(sc["width"], sc["height"])):
            rp = cr.CanvasReplay(be, linear_extension=True)
            for b in sc["bitmaps"]:
                rp.add_bitmap(b)
            rp.render(sc["stage"])
            imgs.append(be.premultiplied_rgba().astype(int)); be.close()
        assert np.array_equal(imgs[0], imgs[1]), (seed, it)


@pytest.mark.parametrize("seed", [21, 22, 23, 24])
def test_radial_gradient_fills(seed):
    """Radial / focal gradients the way the renderer issues them (createRadialGradient(f * 16384, 0, 0, 0, 0, 16384) under the fill
    matrix, 1-8 stops, translucent stops, duplicate offsets, shapes partly off the frame, on a clear frame and over other fills),
    plus general two-circle gradients: cairo's fit-to-range scaling, pixman's 16.16 circles, exact integer B and C, the double root
    and the single-precision colour ramp are all restated -- identical frames."""
    rng = np.random.default_rng(seed)
    painted = 0
    for it in range(60):
        W, H = int(rng.integers(30, 120)), int(rng.integers(30, 100))
        ops = []
        for k in range(int(rng.integers(1, 4))):
            n = int(rng.integers(1, 9))
            offs = np.sort(rng.integers(0, 256, n)) / 255.0
            if n > 2 and rng.integers(0, 3) == 0:
                offs[1] = offs[0]
            stops = [(float(offs[i]), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)),
                      int(rng.choice([255, 255, 128, 0, 37]))) for i in range(n)]
            # the gradient circle (radius 16384 units) is at least 0.6 frame diagonals wide along its short axis and centred
            # inside the frame: every sample then stays within twice the radius, i.e. inside pixman's 16.16 range after cairo's
            # range fitting (beyond that pixman_transform_point_3d fails and the reference stack leaves stale scanline bytes)
            ky = rng.uniform(0.5, 1.0)
            sc = rng.uniform(0.6, 3.0) * 20 / 16384 * float(np.hypot(W, H)) / ky
            t = rng.uniform(-3.2, 3.2)
            c, s_ = np.cos(t), np.sin(t)
            fm = (sc * c * 16384 / 16384, sc * s_, -sc * ky * s_, sc * ky * c, float(rng.integers(0, W * 20)), float(rng.integers(0, H * 20)))
            if rng.integers(0, 4) == 0:   # a general pair of circles in a small pattern space
                circles = (float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), float(rng.uniform(0, 20)),
                           float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), float(rng.uniform(20, 90)))
                fm = (20.0 * c, 20.0 * s_, -20.0 * s_, 20.0 * c, fm[4], fm[5])
            else:
                focal = float(rng.choice([0.0, 0.0, rng.uniform(-0.95, 0.95)]))
                circles = (focal * 16384, 0.0, 0.0, 0.0, 0.0, 16384.0)
            pts = [(int(rng.integers(-300, W * 20 + 300)), int(rng.integers(-300, H * 20 + 300))) for _ in range(int(rng.integers(3, 7)))]
            ops.append((fm, circles, stops, pts))
        imgs = []
        for be in (cb.CairoBackend(W, H), ob.OracleBackend(W, H)):
            be.set_transform_identity(); be.clear_all(); be.scale(1 / 20, 1 / 20)
            for fm, circles, stops, pts in ops:
                be.begin_path(); be.move_to(*pts[0])
                for q in pts[1:]:
                    be.line_to(*q)
                be.line_to(*pts[0])
                be.save(); be.transform(*fm)
                be.set_fill_radial(*circles, stops); be.fill(); be.restore()
            imgs.append(be.premultiplied_rgba().astype(int)); be.close()
        assert np.array_equal(imgs[0], imgs[1]), (seed, it, int(np.abs(imgs[0] - imgs[1]).max()), int((np.abs(imgs[0] - imgs[1]).max(-1) > 0).sum()))
        painted += int((imgs[0][..., 3] > 0).sum())
    assert painted > 20000


@pytest.mark.parametrize("seed", [31, 32])
def test_radial_scenes_through_the_canvas_replay(seed):
    """The scenes of the GPU gradient fuzz (tests/helpers.py rand_radial_scene) rendered by libcairo and by the oracle: identical."""
    from helpers import rand_radial_scene
    from oracle import canvas_replay as cr
    rng = np.random.default_rng(seed)
    for it in range(40):
        sc = rand_radial_scene(rng)
        imgs = []
        for be in (cb.CairoBackend(sc["width"], sc["height"]), ob.OracleBackend(sc["width"], sc["height"])):
            cr.CanvasReplay(be, linear_extension=True).render(sc["stage"])
            imgs.append(be.premultiplied_rgba().astype(int)); be.close()
        assert np.array_equal(imgs[0], imgs[1]), (seed, it)


def test_operation_that_paints_nothing_keeps_the_surface_clear():
    """Soak finding: a stroke whose approximate extents touch the frame while its outline lies outside is NOTHING_TO_DO for Cairo --
    the surface stays "clear", so the next translucent fill is composited with the SOURCE rule (0x7f rounding), not OVER (0x80):
    alpha 128 under coverage 1 gives 0, not 1."""
    from helpers import soak_scene
    from oracle import canvas_replay as cr
    for case in (("mixed", 1000, 382), ("mixed", 1000, 545), ("mixed", 1000, 714), ("bitmap", 1000, 332)):
        sc = soak_scene(*case)
        imgs = []
        for be in (cb.CairoBackend(sc["width"], sc["height"]), ob.OracleBackend(sc["width"], sc["height"])):
            if sc.get("even_odd"):
                be.set_fill_rule(True)
            rp = cr.CanvasReplay(be, linear_extension=True)
            for b in sc.get("bitmaps", []):
                rp.add_bitmap(b)
            rp.render(sc["stage"])
            imgs.append(be.premultiplied_rgba().astype(int)); be.close()
        assert np.array_equal(imgs[0], imgs[1]), case


def _replay_both(sc):
    from oracle import canvas_replay as cr
    imgs = []
    for be in (cb.CairoBackend(sc["width"], sc["height"]), ob.OracleBackend(sc["width"], sc["height"])):
        if sc.get("even_odd"):
            be.set_fill_rule(True)
        rp = cr.CanvasReplay(be, linear_extension=True)
        for b in sc.get("bitmaps", []):
            rp.add_bitmap(b)
        rp.render(sc["stage"])
        imgs.append(be.premultiplied_rgba().astype(int)); be.close()
    return imgs


def test_gradient_whose_centre_of_operation_leaves_16_16_skips_the_translation_fix():
    """Soak finding (large frames): Cairo corrects the rounded pixman matrix's translation so that the centre of the operation's
    rectangle maps exactly -- unless pixman_transform_point_3d cannot represent that centre in 16.16, which happens for gradients
    (scaled into +-16383) whose shape lies more than two radii from the gradient's centre.  Then the translation stays as rounded;
    before this rule 13 of 150 large scenes differed from libcairo in a few pixels by 1/255."""
    from helpers import soak_scene
    sc = soak_scene("big", 300, 9)
    sc["stage"] = {"children": sc["stage"]["children"][29:30]}
    ref, got = _replay_both(sc)
    assert (ref[..., 3] > 0).sum() > 10000 and np.array_equal(ref, got)


def test_gradient_with_only_transparent_stops_is_a_clear_source():
    """Soak finding: a gradient all of whose stops have alpha 0 is a clear source (_cairo_pattern_is_clear): OVER with it is skipped
    before it reaches the surface, which therefore stays "clear" -- and the next translucent fill takes the SOURCE route."""
    from helpers import soak_scene
    sc = soak_scene("big", 5000, 854)
    kids = sc["stage"]["children"]
    sc["stage"] = {"children": [kids[3], kids[11]]}
    ref, got = _replay_both(sc)
    assert (ref[..., 3] > 0).sum() > 1000 and np.array_equal(ref, got)


@pytest.mark.parametrize("linear", [False, True], ids=["exact", "linear"])
def test_dense_scenes_through_the_canvas_replay(linear):
    """The dense mixed-fill frames of tests/helpers.py rand_dense_scene (the GPU instance tests' corpus: dozens of layered solids,
    box paths, bitmap fills magnified and minified, radial and focal gradients, strokes, opaque covers) rendered by libcairo and by
    the oracle: identical; with linear gradients (the documented extension) within +-1 LSB."""
    from helpers import rand_dense_scene
    rng = np.random.default_rng(4040 if not linear else 4041)
    for it in range(12):
        ref, got = _replay_both(rand_dense_scene(rng, linear=linear))
        assert (ref[..., 3] > 0).mean() > 0.9
        if linear:
            assert np.abs(ref - got).max() <= 1, it
        else:
            assert np.array_equal(ref, got), (it, int((ref != got).any(-1).sum()))


def test_gradient_edges_through_the_canvas_replay():
    """Focal points at +-1 and beyond (epsilons +-256 ... 32767, -32768: the a == 0 branch, cones with transparent regions) and 1, 2
    and 16 stops with translucent and duplicate ratios, on a clear frame and over a backdrop (tests/helpers.py
    gradient_edge_scenes; the gradient circle covers the frame): libcairo and the oracle agree byte for byte."""
    from helpers import gradient_edge_scenes
    scenes = gradient_edge_scenes()
    cones = 0
    for key, sc in sorted(scenes.items()):
        ref, got = _replay_both(sc)
        assert np.array_equal(ref, got), key
        assert (ref[..., 3] > 0).sum() > 500, key
        cones += "clear" in key and "focal" in key and bool((ref[..., 3] == 0).any() and (ref[..., 3] > 0).any())
    assert cones > 10
