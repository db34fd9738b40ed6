"""Random frames of one shape filled with a pixman-exact linear gradient, and what each must look like -- for
tests/test_linear_model.py (held against live libcairo, no GPU) and tests/test_linear_fuzz_gpu.py (held against the device).

    cases(spread, size, count)   the seeded generator: the same cases wherever it is called
    expected(case)               linear_model.frame over the shape's coverage (made without libcairo): truth, every_sample, caveat

A case draws
    the gradient   the line (-16384, 0)-(16384, 0) -- what a SWF fill has -- under a matrix that is exactly horizontal (the position
                   stands still from row to row), exactly vertical (every row one colour: pixman's constant-row branch), steep (a few
                   degrees off vertical), rotated or sheared, with a half length of 0.15 to 3 times the shape's width (shorter, the
                   shape leaves pixman's 16.16 range: at most four periods fit into it), 2 to 16 stops out of a pool with repeated
                   ratios, colours opaque, translucent and transparent (tests/spread_fuzz.py, _stops)
    the shape      a box (two in three on whole pixels), a slanted quadrilateral, a random convex polygon, a notched one (rows with two
                   covered runs); its rectangle's left edge is rarely column 0
and is kept if the product accepts it (linear_model.accepted: inside the range, and no row step between 0 and one 16.16 unit).
"""
import math

import numpy as np

import blend_scenes as bs
import linear_model as lm
import linear_scenes as ls
import spread_fuzz as sf
import spread_model as sm
import spread_scenes as ss
from scenarios import _m

SIZES = ((48, 12), (96, 48))
SHAPES = ("box", "quad", "convex", "notched")
KINDS = ("horizontal", "vertical", "steep", "rotated", "sheared")
EXTEND = {"pad": lm.PAD, "reflect": lm.REFLECT, "repeat": lm.REPEAT}
LINE = (-ss.R, 0.0, ss.R, 0.0)


def _matrix(rng, kind, rect):
    x0, y0, x1, y1 = rect
    across = (y1 - y0) if kind in ("vertical", "steep") else (x1 - x0)
    s = across * rng.uniform(0.15, 3.0) * 20 / ss.R
    tx, ty = int(rng.integers(x0 * 20, x1 * 20 + 1)), int(rng.integers(y0 * 20, y1 * 20 + 1))
    if kind == "horizontal":
        return _m(s, s * rng.uniform(0.6, 1.4), tx, ty)
    if kind == "vertical":
        return _m(0.0, 0.0, tx, ty, s, -s * rng.uniform(4.0, 8.0))
    a = rng.uniform(1.45, 1.69) if kind == "steep" else rng.uniform(0.0, 2 * math.pi)
    k = rng.uniform(0.7, 1.3) * (4.0 if kind == "steep" else 1.0)
    shear = s * rng.uniform(-0.4, 0.4) if kind == "sheared" else 0.0
    return _m(s * math.cos(a), s * k * math.cos(a), tx, ty, s * math.sin(a), -s * k * math.sin(a) + shear)


def make_case(W, H, spread, matrix, stops, pts, shape="", **extra):
    fill = ss._fill("linear", matrix, stops, spread)
    rect = sf.pixel_rect(pts, W, H)
    tw = [(round(x * 20), round(y * 20)) for x, y in pts]
    whole_box = shape == "box" and all(x % 20 == 0 and y % 20 == 0 for x, y in tw)
    model = dict(matrices=[matrix], rect=rect, stops=[(t / 255, c[0] / 255, c[1] / 255, c[2] / 255, c[3] / 255) for t, c in stops])
    return dict(width=W, height=H, spread=spread, shape=shape, points=pts, model=model, whole_box=whole_box,
                scene=ss._scene([ss._shape(pts, fill)], W, H), white=ss._scene([bs._shape(pts, (255, 255, 255, 255))], W, H), **extra)


def cases(spread, size, count, seed=9101):
    W, H = size
    rng = np.random.default_rng([ls.SPREADS.index(spread), SIZES.index(tuple(size)), seed])
    out = []
    while len(out) < count:
        shape, kind = SHAPES[len(out) % len(SHAPES)], KINDS[(len(out) // len(SHAPES)) % len(KINDS)]
        pts = sf._points(rng, shape, W, H)
        rect = sf.pixel_rect(pts, W, H)
        matrix = _matrix(rng, kind, rect)
        stops = sf._stops(rng)
        if len(stops) < 2:
            stops = stops + [(255, stops[0][1][::-1])]
        m = sm.pattern_matrix([matrix])
        if m is None or not lm.accepted(m, LINE, rect):
            continue
        out.append(make_case(W, H, spread, matrix, stops, pts, shape, kind=kind, index=len(out)))
    return out


def coverage(case):
    """the shape's coverage, H x W bytes: the alpha of the same outline filled opaque white, through the oracle"""
    from helpers import oracle_render
    return oracle_render(case["white"])[..., 3].copy()


def expected(case, alpha=None):
    md = case["model"]
    alpha = coverage(case) if alpha is None else alpha
    out = lm.frame(sm.pattern_matrix(md["matrices"]), LINE, md["stops"], EXTEND[case["spread"]], md["rect"], alpha,
                   boxes=[md["rect"]] if case["whole_box"] else None)
    out["alpha"] = alpha
    return out
