"""Random frames of one shape filled with a reflected or repeated radial (or focal) gradient, and what each must look like -- for
tests/test_spread_model.py (held against live libcairo, no GPU) and tests/test_spread_fuzz_gpu.py (held against the device).

    cases(spread, kind, aliased, size, count)   the seeded generator: the same cases wherever it is called
    coverage(case)                              the shape's coverage, without libcairo
    expected(case)                              spread_model.frame over that coverage: truth, every_sample, caveat

A case draws
    the gradient   a matrix as tests/test_spread_model.py draws its boxes' (radius 7 to 40 px, squeezed and skewed; every fourth with
                   the centre on a pixel centre and a radius of whole pixels, so that samples fall on stops and seams), a focal point
                   of 1 to 249 epsilons on the kind's side, 1 to 16 stops out of a pool that holds 0, 255 and repeated ratios
                   (coincident stops), colours opaque, translucent and transparent
    the shape      a box (two in three on whole pixels), a slanted quadrilateral, a random convex polygon, a notched polygon and a stepped (rectilinear)
                   one: the last two have rows with two covered runs
    the frame      48 x 12 or 80 x 20: a shape can cross a 64-pixel strip boundary and a 16-row tile boundary
and is kept if the shape's rectangle lies within 1.9 radii of the centre and of the focus (beyond two, libcairo itself paints nothing:
tests/spread_scenes.py).  The operation's rectangle is the shape's pixel extents.
"""
import math

import numpy as np

import blend_scenes as bs
import spread_model as sm
import spread_scenes as ss

SIZES = ((48, 12), (80, 20))
SHAPES = ("box", "quad", "convex", "notched", "stepped")
EXTEND = {"reflect": sm.REFLECT, "repeat": sm.REPEAT}
SIGN = {"radial": 0.0, "focal+": 1.0, "focal-": -1.0}
RATIO_POOL = [0, 0, 51, 102, 128, 204, 255, 255]


def in_range(m, circles, rect):
    """the rectangle maps within pixman's 16.16 range, relative to the centre and to the focus: 1.9 radii (tests/spread_scenes.py)"""
    for x in (rect[0], rect[2]):
        for y in (rect[1], rect[3]):
            u, v = sm.apply(m, float(x), float(y))
            if max(abs(u), abs(v), abs(u - circles[0]), abs(v - circles[1])) > 1.9 * ss.R:
                return False
    return True


def _matrix(rng, W, H):
    radius = rng.uniform(7, 40)
    s = radius * 20 / ss.R
    matrix = ss._m(s, s * rng.uniform(0.6, 1.4), int(rng.integers(4 * 20, (W - 4) * 20)), int(rng.integers(0, H * 20)), s * rng.uniform(-0.4, 0.4), s * rng.uniform(-0.4, 0.4))
    if rng.integers(0, 4) == 0:                  # a centre on a pixel centre and a radius of whole pixels: samples on stops and seams
        radius = int(rng.integers(6, 26))
        s = radius * 20 / ss.R
        matrix = ss._m(s, s, int(rng.integers(6, W - 6)) * 20 + 10, int(rng.integers(2, H - 2)) * 20 + 10)
    return matrix


def _stops(rng):
    n = int(rng.integers(1, 17))
    ratios = sorted(int(v) for v in rng.choice(RATIO_POOL + list(rng.integers(0, 256, 8)), n))
    look = int(rng.integers(0, 3))               # every colour opaque; any alpha; some stops transparent
    out = []
    for t in ratios:
        c = [int(v) for v in rng.integers(0, 256, 4)]
        if look == 0:
            c[3] = 255
        elif look == 2 and rng.integers(0, 3) == 0:
            c[3] = 0
        out.append((t, tuple(c)))
    return out


def _points(rng, shape, W, H):
    """the outline in pixels (it is rounded to twentieths); every shape at least three pixels wide and two high"""
    x0 = int(rng.integers(0, W - 8))
    x1 = int(rng.integers(x0 + 6, W + 1))
    y0 = int(rng.integers(0, H - 4))
    y1 = int(rng.integers(y0 + 3, H + 1))
    if shape == "box":                           # every third one off the pixel grid: boxes with partial coverage, composited through a mask
        if rng.integers(0, 3) == 0:
            j = lambda: int(rng.integers(1, 20)) / 20
            return ss._box(x0 + j(), y0 + j(), x1 - j(), y1 - j())
        return ss._box(x0, y0, x1, y1)
    if shape == "quad":
        return ss._quad(x0, y0, x1, y1)
    cx, cy, rx, ry = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2, (y1 - y0) / 2
    if shape == "convex":
        n = int(rng.integers(3, 8))
        ang = np.sort(rng.uniform(0, 2 * math.pi, n) + np.arange(n) * 1e-3)
        return [(cx + rx * math.cos(a), cy + ry * math.sin(a)) for a in ang]
    xa = x0 + (x1 - x0) * rng.uniform(0.1, 0.4)
    xb = x0 + (x1 - x0) * rng.uniform(0.6, 0.9)
    ym = y0 + (y1 - y0) * rng.uniform(0.4, 0.9)
    if shape == "notched":                       # a notch from the top edge: the rows above its tip have two covered runs
        j = lambda: rng.uniform(0.0, 0.9)
        return [(x0 + j(), y0 + j()), (xa, y0 + j()), ((xa + xb) / 2 + j(), ym), (xb, y0 + j()), (x1 - j(), y0 + j()), (x1 - j(), y1 - j()), (x0 + j(), y1 - j())]
    assert shape == "stepped"                    # whole pixels: two prongs above a bar, or (every other one) a bar above two prongs
    xa, xb, ym = int(round(xa)), int(round(xb)), min(max(int(round(ym)), y0 + 1), y1 - 1)
    xa, xb = max(xa, x0 + 1), min(max(xb, xa + 1), x1 - 1)
    if rng.integers(0, 2):
        return [(x0, y0), (xa, y0), (xa, ym), (xb, ym), (xb, y0), (x1, y0), (x1, y1), (x0, y1)]
    return [(x0, y0), (x1, y0), (x1, y1), (xb, y1), (xb, ym), (xa, ym), (xa, y1), (x0, y1)]


def pixel_rect(pts, W, H):
    """the pixel extents of an outline given in pixels, as the scene holds it (in twentieths), inside the frame"""
    xs, ys = [round(x * 20) for x, _ in pts], [round(y * 20) for _, y in pts]
    return (max(min(xs) // 20, 0), max(min(ys) // 20, 0), min(-(-max(xs) // 20), W), min(-(-max(ys) // 20), H))


def piecewise(pts, aliased):
    """libcairo composites the outline piece by piece, each a scanline of its own for pixman: span by span when aliased, box by box when
    the outline is rectilinear on whole pixels -- and otherwise once, through a mask"""
    tw = [(round(x * 20), round(y * 20)) for x, y in pts]
    boxes = all(x % 20 == 0 and y % 20 == 0 for x, y in tw) and all(a[0] == b[0] or a[1] == b[1] for a, b in zip(tw, tw[1:] + tw[:1]))
    return bool(aliased) or boxes


def make_case(W, H, aliased, spread, kind, matrix, epsilons, stops, pts, shape="", **extra):
    """a case from its parts: `stops` is [(ratio 0..255, (r, g, b, a) bytes)], `pts` the outline in pixels"""
    fill = ss._fill(kind, matrix, stops, spread)
    if kind != "radial":
        fill["focal_point"] = {"epsilons": int(epsilons)}
    model = dict(matrices=[matrix], circles=(epsilons / 256.0 * ss.R, 0.0, 0.0, 0.0, 0.0, ss.R), rect=pixel_rect(pts, W, H),
                 stops=[(t / 255, c[0] / 255, c[1] / 255, c[2] / 255, c[3] / 255) for t, c in stops])
    return dict(width=W, height=H, aliased=bool(aliased), spread=spread, kind=kind, shape=shape, points=pts, model=model, per_run=piecewise(pts, aliased),
                scene=ss._scene([ss._shape(pts, fill)], W, H), white=ss._scene([bs._shape(pts, (255, 255, 255, 255))], W, H), **extra)


def cases(spread, kind, aliased, size, count, seed=7001):
    """`count` cases of one spread, gradient kind, antialias mode and frame size; the shapes take turns"""
    W, H = size
    rng = np.random.default_rng([ss.SPREADS.index(spread), ss.KINDS.index(kind), int(aliased), SIZES.index(tuple(size)), seed])
    out = []
    while len(out) < count:
        shape = SHAPES[len(out) % len(SHAPES)]
        matrix = _matrix(rng, W, H)
        epsilons = int(SIGN[kind] * int(rng.integers(1, 250)))
        stops = _stops(rng)
        pts = _points(rng, shape, W, H)
        m = sm.pattern_matrix([matrix])
        rect = pixel_rect(pts, W, H)
        if m is None or not in_range(m, (epsilons / 256.0 * ss.R, 0.0), rect):
            continue
        out.append(make_case(W, H, aliased, spread, kind, matrix, epsilons, stops, pts, shape, index=len(out)))
    return out


def coverage(case):
    """The shape's coverage, H x W bytes: the alpha of the same outline filled opaque white -- antialiased, through the oracle; aliased,
    where there is no oracle, tests/frame_model.py's exact model of the aliased rule over the frame builder's arrays."""
    if case["aliased"]:
        import frame_model as fm
        from host_frames import build_on_host
        return fm.render(*build_on_host(case["white"], True), case["width"], case["height"], aliased=True)[..., 3].copy()
    from helpers import oracle_render
    return oracle_render(case["white"])[..., 3].copy()


def expected(case, alpha=None):
    """spread_model.frame of the case: dict(truth, every_sample, caveat) plus alpha"""
    md = case["model"]
    alpha = coverage(case) if alpha is None else alpha
    out = sm.frame(sm.pattern_matrix(md["matrices"]), md["circles"], md["stops"], EXTEND[case["spread"]], md["rect"], alpha, case["per_run"])
    out["alpha"] = alpha
    return out


def crossings(case):
    """(the rectangle crosses the 64-pixel strip boundary, the 16-row tile boundary)"""
    x0, y0, x1, y1 = case["model"]["rect"]
    return x0 < 64 < x1, y0 < 16 < y1
