import json
import os

import numpy as np

from oracle import canvas_replay as cr, oracle_backend as ob

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FIX = os.path.join(GOLD, "fixtures")


def fixture(name):
    with open(os.path.join(FIX, name + ".ast.json")) as f:
        return json.load(f)


def fixture_text(name):
    with open(os.path.join(FIX, name)) as f:
        return f.read()


def golden(name, key):
    return np.load(os.path.join(GOLD, name + ".npz"))[key]


def oracle_render(sc):
    """premultiplied RGBA of a tests/scenarios.py scenario through the CPU restatement"""
    be = ob.OracleBackend(sc["width"], sc["height"])
    if sc.get("even_odd"):
        be.set_fill_rule(True)
    rp = cr.CanvasReplay(be, linear_extension=True)
    for b in sc.get("bitmaps", []):
        rp.add_bitmap(b)
    rp.render(sc["stage"])
    out = be.premultiplied_rgba()
    unsupported = be.unsupported
    be.close()
    assert not unsupported, "scenario uses stroker features outside the restated subset"
    return out


def product_render(sc, stats=None, **kw):
    """premultiplied RGBA of a scenario through libswfr.so (HIP path); `stats` (a dict) collects the handle's swfr_stats"""
    import swf_renderer_amd as S
    r = S.Renderer(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")), **kw)
    try:
        for b in sc.get("bitmaps", []):
            r.add_bitmap(b)
        try:
            r.render(sc["stage"])
        finally:
            if stats is not None:
                for k, v in r.stats().items():
                    stats[k] = stats.get(k, 0) + v
        return r.read_image(premultiplied=True)
    finally:
        r.close()


def diff_stats(a, b):
    d = (a != b).any(-1)
    mx = int(np.abs(a.astype(int) - b.astype(int)).max()) if d.any() else 0
    return int(d.sum()), mx


# ---- the reference's own acceptance metric (ts/src/test/node-canvas-renderer.spec.ts:54-65: pixelmatch, threshold 0.05,
#      anti-aliased pixels skipped, at most 1e-4 of the pixels may differ) restated for reporting
def _pm_delta(p1, p2, y_only=False):
    r1, g1, b1, a1 = (float(v) for v in p1)
    r2, g2, b2, a2 = (float(v) for v in p2)
    if (r1, g1, b1, a1) == (r2, g2, b2, a2):
        return 0.0
    if a1 < 255:
        a1 /= 255; r1, g1, b1 = 255 + (r1 - 255) * a1, 255 + (g1 - 255) * a1, 255 + (b1 - 255) * a1
    if a2 < 255:
        a2 /= 255; r2, g2, b2 = 255 + (r2 - 255) * a2, 255 + (g2 - 255) * a2, 255 + (b2 - 255) * a2
    y = (r1 * 0.29889531 + g1 * 0.58662247 + b1 * 0.11448223) - (r2 * 0.29889531 + g2 * 0.58662247 + b2 * 0.11448223)
    if y_only:
        return y
    i = (r1 * 0.59597799 - g1 * 0.27417610 - b1 * 0.32180189) - (r2 * 0.59597799 - g2 * 0.27417610 - b2 * 0.32180189)
    q = (r1 * 0.21147017 - g1 * 0.52261711 + b1 * 0.31113672) - (r2 * 0.21147017 - g2 * 0.52261711 + b2 * 0.31113672)
    return 0.5053 * y * y + 0.299 * i * i + 0.1957 * q * q


def _pm_many_siblings(img, x1, y1):
    h, w = img.shape[:2]
    zeroes = 1 if (x1 == 0 or y1 == 0 or x1 == w - 1 or y1 == h - 1) else 0
    for x in range(max(x1 - 1, 0), min(x1 + 1, w - 1) + 1):
        for y in range(max(y1 - 1, 0), min(y1 + 1, h - 1) + 1):
            if (x, y) != (x1, y1) and (img[y, x] == img[y1, x1]).all():
                zeroes += 1
                if zeroes > 2:
                    return True
    return False


def _pm_antialiased(img, x1, y1, img2):
    h, w = img.shape[:2]
    zeroes = 1 if (x1 == 0 or y1 == 0 or x1 == w - 1 or y1 == h - 1) else 0
    mn = mx = 0.0
    mnp = mxp = None
    for x in range(max(x1 - 1, 0), min(x1 + 1, w - 1) + 1):
        for y in range(max(y1 - 1, 0), min(y1 + 1, h - 1) + 1):
            if (x, y) == (x1, y1):
                continue
            d = _pm_delta(img[y1, x1], img[y, x], True)
            if d == 0:
                zeroes += 1
                if zeroes > 2:
                    return False
            elif d < mn:
                mn, mnp = d, (x, y)
            elif d > mx:
                mx, mxp = d, (x, y)
    if mn == 0 or mx == 0:
        return False
    return ((_pm_many_siblings(img, *mnp) and _pm_many_siblings(img2, *mnp)) or
            (_pm_many_siblings(img, *mxp) and _pm_many_siblings(img2, *mxp)))


def pixelmatch_count(a, b, threshold=0.05):
    """Number of mismatched pixels as the reference's spec counts them (straight RGBA8 images of equal shape)."""
    assert a.shape == b.shape
    max_delta = 35215 * threshold * threshold
    ys, xs = np.nonzero((a != b).any(-1))
    n = 0
    for y, x in zip(ys.tolist(), xs.tolist()):
        if _pm_delta(a[y, x], b[y, x]) > max_delta:
            if not (_pm_antialiased(a, x, y, b) or _pm_antialiased(b, x, y, a)):
                n += 1
    return n


# ---- the Rust decoder's golden format (rs/src/decoder/shape_decoder.rs: `format!("{:#?}\n", shape)` of Shape { paths:
#      Vec<StyledPath { path: lyon Path, fill: Option<FillStyle>, line: Option<LineStyle> }> }, rs/src/lib.rs:26-71)
def shape_to_rs_log(decoded: dict, ast: dict) -> str:
    """Pretty Debug text of the Rust `Shape` for a decoded shape (the product's swfr_shape_json output, straight lines and
    solid styles only, as in the three fixtures the Rust test holds); line-style attributes the TS form drops come from the AST."""
    def ind(n):
        return "    " * n

    def solid(color, n):
        c = [int(round(color[k] * 255)) for k in "rgba"]
        return [ind(n) + "Solid(", ind(n + 1) + "Solid {", ind(n + 2) + "color: StraightSRgba8 {",
                ind(n + 3) + "r: %d," % c[0], ind(n + 3) + "g: %d," % c[1], ind(n + 3) + "b: %d," % c[2], ind(n + 3) + "a: %d," % c[3],
                ind(n + 2) + "},", ind(n + 1) + "},", ind(n) + "),"]

    out = ["Shape {", ind(1) + "paths: ["]
    for p in decoded["paths"]:
        pts, verbs = [], []
        for c in p["commands"]:
            if c["type"] == 2:
                pts.append((c["x"], c["y"])); verbs.append("MoveTo")
            elif c["type"] == 0:
                pts.append((c["endX"], c["endY"])); verbs.append("LineTo")
            else:
                raise ValueError("the Rust decoder of the reference handles straight edges only")
        out += [ind(2) + "StyledPath {", ind(3) + "path: Path {", ind(4) + "points: ["]
        out += [ind(5) + "(%.1f,%.1f)," % (x, y) for x, y in pts]
        out += [ind(4) + "],", ind(4) + "verbs: ["]
        out += [ind(5) + v + "," for v in verbs]
        out += [ind(4) + "],", ind(3) + "},"]
        if "fill" in p:
            out += [ind(3) + "fill: Some("] + solid(p["fill"]["color"], 4) + [ind(3) + "),"]
        else:
            out.append(ind(3) + "fill: None,")
        if "line" in p:
            ls = next(l for l in ast["shape"]["initial_styles"]["line"] if l["width"] == p["line"]["width"])
            cap = lambda v: v.capitalize()
            out += [ind(3) + "line: Some(", ind(4) + "LineStyle {", ind(5) + "width: %d," % ls["width"],
                    ind(5) + "start_cap: %s," % cap(ls["start_cap"]), ind(5) + "end_cap: %s," % cap(ls["end_cap"]),
                    ind(5) + "join: %s," % cap(ls["join"]["type"])]
            out += [ind(5) + "%s: %s," % (k, "true" if ls[k] else "false") for k in ("no_h_scale", "no_v_scale", "no_close", "pixel_hinting")]
            out += [ind(5) + "fill: " + solid(p["line"]["fill"]["color"], 5)[0].strip()] + solid(p["line"]["fill"]["color"], 5)[1:]
            out += [ind(4) + "},", ind(3) + "),"]
        else:
            out.append(ind(3) + "line: None,")
        out.append(ind(2) + "},")
    out += [ind(1) + "],", "}"]
    return "\n".join(out) + "\n"


def make_bitmap_tag(bitmap_id, width, height, rng, colors=64):
    """A random DefineBitmap in the only format the reference decodes (image/x-swf-bmp, format 3: zlib-compressed colour table +
    8-bit indices, rows padded to 4; decode-x-swf-bmp.ts:9-41)."""
    import zlib
    table = rng.integers(0, 256, (colors, 3)).astype(np.uint8)
    padded = width + ((4 - (width % 4)) % 4)
    idx = np.zeros((height, padded), np.uint8)
    idx[:, :width] = rng.integers(0, colors, (height, width))
    body = zlib.compress(table.tobytes() + idx.tobytes())
    data = bytes([3, width & 255, width >> 8, height & 255, height >> 8, colors - 1]) + body
    return {"type": "define-bitmap", "id": bitmap_id, "width": width, "height": height, "media_type": "image/x-swf-bmp", "data": data.hex()}


def large_texture_scene(width=3840, height=2160, tex=4096, seed=99):
    """BASELINE.json config 4's HBM-bound variant: a frame-filling rectangle with a tex x tex bitmap fill sampled
    at width / tex pixels per texel (bilinear: every texel of the visible part is fetched about once, nothing stays in a cache)."""
    import scenarios
    rng = np.random.default_rng(seed)
    bmp = make_bitmap_tag(9, tex, tex, rng, colors=256)
    k = width / tex
    fill = {"type": "bitmap", "bitmap_id": 9, "repeating": False, "smoothed": True, "matrix": scenarios._m(20 * k, 20 * k, 0, 0)}
    pts = np.array([(0, 0), (width, 0), (width, height), (0, height)], float)
    return dict(width=width, height=height, bitmaps=[bmp], stage={"children": [{"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), fill)}]})


def rand_bitmap_scene(rng):
    """One random frame of bitmap-filled shapes as the renderer draws them: repeat / no-repeat fills from 20x minified to 30x
    magnified, rotated, reflected, partly off-frame, polygons and (un)aligned rectangles, with translucent solids in between."""
    import scenarios
    W, H = int(rng.integers(40, 200)), int(rng.integers(40, 140))
    bmp = make_bitmap_tag(3, int(rng.integers(1, 48)), int(rng.integers(1, 48)), rng)
    kids = []
    for _ in range(int(rng.integers(1, 4))):
        if rng.integers(0, 4) == 0:
            pts = rng.uniform(0, 1, (4, 2)) * [W, H]
            kids.append({"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": scenarios._rgba(30, 200, 90, int(rng.choice([255, 140])))})})
            continue
        lo, hi = [(0.05, 0.74), (0.3, 3.0), (0.76, 8.0), (10, 30)][int(rng.integers(0, 4))]
        k = float(rng.uniform(lo, hi))
        t = float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 3) else 0.0
        c, sn = np.cos(t), np.sin(t)
        flip = -1.0 if rng.integers(0, 5) == 0 else 1.0
        fill = {"type": "bitmap", "bitmap_id": 3, "repeating": bool(rng.integers(0, 2)), "smoothed": True,
                "matrix": scenarios._m(20 * k * c * flip, 20 * k * c, int(rng.integers(-200, W * 12)), int(rng.integers(-200, H * 12)), 20 * k * sn * flip, -20 * k * sn)}
        kind = int(rng.integers(0, 3))
        if kind == 0:
            pts = rng.uniform(-0.2, 1.2, (int(rng.integers(3, 7)), 2)) * [W, H]
        elif kind == 1:
            x0, y0 = rng.uniform(0, W / 2), rng.uniform(0, H / 2)
            x1, y1 = x0 + rng.uniform(3, W), y0 + rng.uniform(3, H)
            pts = np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
        else:
            x0, y0 = int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2))
            x1, y1 = x0 + int(rng.integers(1, W)), y0 + int(rng.integers(1, H))
            pts = np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], float)
        mat = scenarios._m(float(rng.choice([1, 1, 0.7, 1.6])), float(rng.choice([1, 1, 1.3])), int(rng.integers(-200, 300)), int(rng.integers(-200, 300)))
        kids.append({"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), fill), "matrix": mat})
    return dict(width=W, height=H, bitmaps=[bmp], stage={"children": kids})


def rand_radial_scene(rng):
    """One random frame of shapes with radial / focal gradient fills as the reference draws them (fill matrix maps the +-16384
    gradient box onto the shape), 1-8 stops with translucent colours and duplicate ratios, on a clear frame and over each other.
    The gradient circle is at least 0.6 frame diagonals wide and centred in the frame: samples stay inside pixman's 16.16 range."""
    import scenarios
    W, H = int(rng.integers(40, 200)), int(rng.integers(40, 140))
    kids = []
    for _ in range(int(rng.integers(1, 4))):
        n = int(rng.integers(1, 9))
        ratios = sorted(int(v) for v in rng.integers(0, 256, n))
        if n > 2 and rng.integers(0, 3) == 0:
            ratios[1] = ratios[0]
        colors = [(ratios[i], (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.choice([255, 255, 128, 0, 37])))) for i in range(n)]
        ky = float(rng.uniform(0.5, 1.0))
        sc = float(rng.uniform(0.6, 3.0)) * 20 / 16384 * float(np.hypot(W, H)) / ky
        t = float(rng.uniform(-3.2, 3.2))
        c, sn = np.cos(t), np.sin(t)
        fill = {"type": "focal-gradient" if rng.integers(0, 2) else "radial-gradient", "gradient": scenarios._grad(colors),
                "matrix": scenarios._m(sc * c, sc * ky * c, int(rng.integers(0, W * 20)), int(rng.integers(0, H * 20)), sc * sn, -sc * ky * sn)}
        if fill["type"] == "focal-gradient":
            fill["focal_point"] = {"epsilons": int(rng.integers(-240, 241))}   # Sfixed8P8: -0.94 .. 0.94
        pts = rng.uniform(-0.1, 1.1, (int(rng.integers(3, 7)), 2)) * [W, H]
        kids.append({"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), fill)})
    return dict(width=W, height=H, stage={"children": kids})


def rand_mixed_scene(rng):
    """solid polygons (both fill rules, translucent), strokes of every style, morph shapes"""
    import scenarios
    from test_host import _rand_path_shape
    W, H = int(rng.integers(40, 260)), int(rng.integers(40, 180))
    kids = []
    for _ in range(int(rng.integers(1, 6))):
        k = int(rng.integers(0, 3))
        if k == 0:
            n = int(rng.integers(3, 10))
            mode = int(rng.integers(0, 4))
            if mode == 0: pts = rng.uniform(0, 1, (n, 2)) * [W, H]
            elif mode == 1: pts = rng.integers(0, 4 * min(W, H), (n, 2)) / 4.0
            elif mode == 2: pts = rng.integers(0, min(W, H), (n, 2)).astype(float)
            else: pts = rng.uniform(-40, 40 + max(W, H), (n, 2))
            col = scenarios._rgba(*[int(v) for v in rng.integers(0, 256, 3)], int(rng.choice([255, 255, 200, 128, 31, 1])))
            kids.append({"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": col})})
        else:
            morph = k == 2
            tag = _rand_path_shape(rng, int(rng.choice([1, 2, 5, 20, 45, 90, 200])), morph)
            sx, sy = float(rng.choice([1, 1, 0.6, 1.7, -1])), float(rng.choice([1, 1, 0.8, 1.3]))
            mat = scenarios._m(sx, sy, int(rng.integers(-300, 900)) + (2000 if sx < 0 else 0), int(rng.integers(-300, 500)),
                               float(rng.choice([0, 0, 0.2])), float(rng.choice([0, 0, -0.15])))
            kids.append({"type": "morph-shape", "definition": tag, "ratio": float(rng.uniform(0, 1)), "matrix": mat} if morph else
                        {"type": "shape", "definition": tag, "matrix": mat})
    return dict(width=W, height=H, even_odd=bool(rng.integers(0, 2)), stage={"children": kids})




def rand_big_scene(rng):
    """A large frame (several hundred tiles) with dozens of overlapping shapes of every kind: the 64-row chunks of the fused row
    kernel, long band lists, occlusion culling and the shaded tile kernel all at once."""
    import scenarios
    W, H = int(rng.integers(500, 1300)), int(rng.integers(400, 900))
    bmp = make_bitmap_tag(3, int(rng.integers(8, 64)), int(rng.integers(8, 64)), rng)
    kids = []
    for _ in range(int(rng.integers(15, 50))):
        kind = int(rng.integers(0, 10))
        if kind < 5:
            sub = rand_mixed_scene(rng)
        elif kind < 8:
            sub = rand_bitmap_scene(rng)
        else:
            sub = rand_radial_scene(rng)
        k = sub["stage"]["children"][int(rng.integers(0, len(sub["stage"]["children"])))]
        k = dict(k)
        sc = float(rng.choice([1.0, 2.5, 4.0, 7.0]))
        m0 = k.get("matrix") or scenarios._m()
        tx, ty = int(rng.integers(-200, W * 20 - 200)), int(rng.integers(-200, H * 20 - 200))
        # outer placement: scale the child's own matrix and move it somewhere in the big frame
        k["matrix"] = {"scale_x": int(m0["scale_x"] * sc), "scale_y": int(m0["scale_y"] * sc), "rotate_skew0": int(m0["rotate_skew0"] * sc),
                       "rotate_skew1": int(m0["rotate_skew1"] * sc), "translate_x": int(m0["translate_x"] * sc) + tx, "translate_y": int(m0["translate_y"] * sc) + ty}
        kids.append(k)
    return dict(width=W, height=H, bitmaps=[bmp], stage={"children": kids})


def rand_long_scene(rng):
    """Strokes of 40 to 150 segments (round joins and caps when the shape is a morph shape): outlines of many hundred to a few
    thousand edges in ONE path -- the row kernels' larger routines, and the tie-order reconstruction over long edge lists."""
    import scenarios
    from test_host import _rand_path_shape
    W, H = int(rng.integers(250, 700)), int(rng.integers(200, 500))
    kids = []
    for _ in range(int(rng.integers(1, 4))):
        morph = bool(rng.integers(0, 3))
        tag = _rand_path_shape(rng, int(rng.choice([20, 45, 90, 200])), morph, segments=(40, 150))
        sx = float(rng.choice([1, 1.7, 2.5]))
        mat = scenarios._m(sx, sx * float(rng.choice([1, 0.8, 1.3])), int(rng.integers(-300, W * 10)), int(rng.integers(-300, H * 10)),
                           float(rng.choice([0, 0, 0.2])), float(rng.choice([0, 0, -0.15])))
        kids.append({"type": "morph-shape", "definition": tag, "ratio": float(rng.uniform(0, 1)), "matrix": mat} if morph else
                    {"type": "shape", "definition": tag, "matrix": mat})
    return dict(width=W, height=H, even_odd=bool(rng.integers(0, 2)), stage={"children": kids})


# scenes of the soak whose tied edges once came out wrong (tests/test_gpu_parity.py::test_soak_regressions_tied_edges)
SOAK_TIE_CASES = [("radial", 1000, 940), ("mixed", 1000, 445), ("mixed", 1000, 607), ("mixed", 1000, 688), ("bitmap", 1000, 820),
                  ("mixed", 2000, 755), ("mixed", 2000, 1130), ("mixed", 2000, 1265), ("mixed", 4000, 241), ("mixed", 4000, 1424),
                  ("mixed", 5000, 507), ("radial", 7000, 670), ("bitmap", 7000, 816), ("mixed", 7000, 101), ("mixed", 7000, 388),
                  ("mixed", 8000, 995), ("mixed", 8000, 1018), ("mixed", 23000, 196), ("big", 300, 146), ("big", 300, 9), ("big", 5000, 854),
                  ("long", 300, 171), ("mixed", 777777, 722)]


def soak_scene(name, seed, index):
    """Scene `index` of generator `name` in tools/soak.py's numbering (the generators are seeded per name)."""
    gens = {"mixed": rand_mixed_scene, "bitmap": rand_bitmap_scene, "radial": rand_radial_scene, "big": rand_big_scene, "long": rand_long_scene}
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    for _ in range(index + 1):
        sc = gens[name](rng)
    return sc


# ---- the limits of the 24.8 device range the product accepts (+-32768 px = +-2^23 in 24.8): vertices thousands of pixels off the
#      frame, edges tens of thousands of pixels long, 1/256 px slopes across the whole range, end points exactly on the limit
LARGE_MODES = ("far", "long_shallow", "long_steep", "boundary")
LIMIT = 32768.0
EPS = 1.0 / 256


def large_pts(rng, W, H, n, mode):
    """n vertices (device pixels) of a polygon in one of LARGE_MODES around a W x H frame."""
    def inside():
        return (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
    if mode == "far":               # uniform in +-32000 px; the first edge crosses the frame from far left to far right
        pts = [(float(rng.uniform(-32000, -W)), float(rng.uniform(0, H))), (float(rng.uniform(W, 32000)), float(rng.uniform(0, H)))]
        pts += [(float(rng.uniform(-32000, 32000)), float(rng.uniform(-32000, 32000))) for _ in range(n - 2)]
    elif mode == "long_shallow":    # more than 60 000 px wide, less than 1 px tall, through the frame; the rest above or below it
        y = float(rng.uniform(0, H))
        pts = [(float(rng.uniform(-LIMIT, -30000)), y), (float(rng.uniform(30000, LIMIT)), y + float(rng.integers(1, 256)) * EPS * rng.choice([-1, 1]))]
        side = rng.choice([-1, 1])
        pts += [(float(rng.uniform(-LIMIT, LIMIT)), y + side * float(rng.uniform(1, LIMIT - H))) for _ in range(n - 2)]
    elif mode == "long_steep":      # the mirror case; sometimes an edge 1/256 px wide over the whole y range
        x = float(rng.uniform(0, W))
        if rng.integers(0, 2):
            pts = [(x, -LIMIT), (x + EPS * rng.choice([-1, 1]), LIMIT)]
        else:
            pts = [(x, float(rng.uniform(-LIMIT, -30000))), (x + float(rng.integers(1, 256)) * EPS * rng.choice([-1, 1]), float(rng.uniform(30000, LIMIT)))]
        side = rng.choice([-1, 1])
        pts += [(x + side * float(rng.uniform(1, LIMIT - W)), float(rng.uniform(-LIMIT, LIMIT))) for _ in range(n - 2)]
    else:                           # "boundary": coordinates exactly at +-32768 px and +-(32768 - 1/256) px, the others in the frame
        edge = [-LIMIT, -LIMIT + EPS, LIMIT - EPS, LIMIT]
        pts = []
        for _ in range(n):
            x, y = inside()
            if rng.integers(0, 3):
                x = float(rng.choice(edge))
            if rng.integers(0, 3):
                y = float(rng.choice(edge))
            pts.append((x, y))
    return pts


# Shapes of the extreme scenes are given in 1/256 twips (object matrix scale 1/256, exact in 16.16): every 24.8 device position up
# to +-32768 px, the limit included, is then a whole number of shape units.
FINE = 20 * 256


def _fine_shape(pts_px, curves, fill, line=None, line_width_px=0.0, closed=True):
    """DefineShape of one path through device-pixel points (a curve flag at i makes pts[i] the control point of pts[i + 1])."""
    p = [(int(round(x * FINE)), int(round(y * FINE))) for x, y in pts_px]
    sc = {"type": "style-change", "move_to": {"x": p[0][0], "y": p[0][1]}}
    if fill is not None:
        sc["left_fill"] = 1
    if line is not None:
        sc["line_style"] = 1
    recs, cur, i = [sc], p[0], 1
    seq = p[1:] + ([p[0]] if closed else [])
    while i <= len(seq):
        q = seq[i - 1]
        if curves and i < len(seq) and curves[i]:
            e = seq[i]
            recs.append({"type": "edge", "control_delta": {"x": q[0] - cur[0], "y": q[1] - cur[1]}, "delta": {"x": e[0] - cur[0], "y": e[1] - cur[1]}})
            cur, i = e, i + 2
        else:
            recs.append({"type": "edge", "delta": {"x": q[0] - cur[0], "y": q[1] - cur[1]}})
            cur, i = q, i + 1
    xs, ys = [q[0] for q in p], [q[1] for q in p]
    lines = [] if line is None else [{"width": int(round(line_width_px * FINE)), "fill": {"type": "solid", "color": line}}]
    return {"id": 1, "bounds": {"x_min": min(xs), "x_max": max(xs), "y_min": min(ys), "y_max": max(ys)},
            "shape": {"initial_styles": {"fill": [] if fill is None else [fill], "line": lines}, "records": recs}}


def extreme_scene(rng, W, H, mode, kinds=("fill", "curve", "stroke", "rect_stroke")):
    """One frame of one to three shapes whose geometry reaches the limits of the device range (LARGE_MODES): solid fills (opaque and
    translucent, both fill rules), quadratic curves, strokes of the same outlines, and rectilinear strokes whose corners lie near
    +-32768 px."""
    import scenarios
    fine = scenarios._m(1 / 256, 1 / 256)
    kids = []
    for _ in range(int(rng.integers(1, 4))):
        kind = kinds[int(rng.integers(0, len(kinds)))]
        col = scenarios._rgba(*[int(v) for v in rng.integers(0, 256, 3)], int(rng.choice([255, 255, 200, 128, 31])))
        n = int(rng.integers(3, 8))
        pts = large_pts(rng, W, H, n, mode)
        if kind == "fill":
            tag = _fine_shape(pts, None, {"type": "solid", "color": col})
        elif kind == "curve":
            tag = _fine_shape(pts, [bool(rng.integers(0, 2)) for _ in range(n)], {"type": "solid", "color": col})
        elif kind == "stroke":
            # the outline of a polygon stroke keeps the end points of its lines when it is clipped: they must stay inside the
            # range, so the path is pulled in by the miter reach (10 half widths); see test_polygon_stroke_beyond_the_limit_is_refused
            w = float(rng.choice([0.5, 1.0, 3.0, 20.0, 300.0]))
            f = (LIMIT - 5 * w - 1) / LIMIT
            tag = _fine_shape([(x * f, y * f) for x, y in pts], None, None, line=col, line_width_px=w)
        else:                              # axis-aligned outline: Cairo's box stroker, boxes reaching past the frame and the limit
            x0, x1 = sorted(float(v) for v in rng.choice([-LIMIT, -LIMIT + EPS, -30000.0, LIMIT - 50, LIMIT - EPS, LIMIT], 2, replace=False))
            y0, y1 = sorted(float(v) for v in rng.choice([-LIMIT, -LIMIT + EPS, -30000.0, LIMIT - 40, LIMIT - EPS, LIMIT], 2, replace=False))
            if rng.integers(0, 2):         # one side inside the frame: a partly covered frame
                if rng.integers(0, 2):
                    x1 = float(rng.integers(1, W))
                else:
                    y0 = float(rng.integers(0, H - 1))
            tag = _fine_shape([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], None, None, line=col, line_width_px=float(rng.choice([1.0, 2.5, 20.0, 164.0])))
        kids.append({"type": "shape", "definition": tag, "matrix": fine})
    return dict(width=W, height=H, even_odd=bool(rng.integers(0, 2)), stage={"children": kids})


# ---- scene builders shared by the GPU parity tests and tests/test_gpu_instances.py (the same frames under every kernel instance)
def oracle_polys(fx, cols, W, H, even_odd=False):
    """The oracle's frame of polygons given in 24.8 fixed point (synth.scene / synth.twips_to_fixed) with straight RGBA colours."""
    L = ob.lib()
    ctx = L.swfo_create(W, H)
    argb = ((cols[:, 3].astype(np.uint32) << 24) | (cols[:, 0].astype(np.uint32) << 16) |
            (cols[:, 1].astype(np.uint32) << 8) | cols[:, 2]).astype(np.uint32)
    counts = np.full(len(fx), fx.shape[1], dtype=np.int32)
    xy = np.ascontiguousarray(fx.reshape(-1))
    L.swfo_fill_polygons_fixed(ctx, xy.ctypes.data, counts.ctypes.data, argb.ctypes.data, len(fx), 1 if even_odd else 0)
    px = np.ctypeslib.as_array(L.swfo_pixels(ctx), shape=(H, W)).copy()
    L.swfo_destroy(ctx)
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255, px >> 24], -1).astype(np.uint8)


def synth_scene(cfg):
    """(W, H, fixed-point polygons, colours, (edges, paths, styles)) of a swf_renderer_amd.synth configuration (S1, S2, ...)."""
    from swf_renderer_amd import api, synth
    pts, cols = synth.scene(**cfg)
    W, H = cfg["width"], cfg["height"]
    fx = synth.twips_to_fixed(pts)
    return W, H, fx, cols, api.polygons_to_scene(fx, cols, W, H)


TWENTY_THOUSAND_PATHS = dict(seed=77, n_shapes=20000, width=640, height=48, rmin=2.0, rmax=9.0)


def rand_polygon_scene(rng, it):
    """One frame of the polygon fuzz: a random polygon (mode it % 4: uniform, quarter-pixel ties, pixel corners, leaving the frame),
    either fill rule.  Returns (scene, (mode, even_odd, points))."""
    import scenarios
    W, H = int(rng.integers(16, 200)), int(rng.integers(16, 120))
    n = int(rng.integers(3, 9))
    mode = it % 4
    if mode == 0:
        pts = rng.uniform(0, 1, (n, 2)) * [W, H]
    elif mode == 1:
        pts = rng.integers(0, 4 * min(W, H), (n, 2)) / 4.0          # tie-heavy quarter pixels
    elif mode == 2:
        pts = rng.integers(0, min(W, H), (n, 2)).astype(float)      # vertices on pixel corners
    else:
        pts = rng.uniform(-30, 30 + max(W, H), (n, 2))              # leaves the frame
    eo = bool(rng.integers(0, 2))
    col = scenarios._rgba(int(rng.integers(0, 256)), 9, 200, int(rng.choice([255, 255, 120])))
    tag = scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": col})
    return dict(width=W, height=H, even_odd=eo, stage={"children": [{"type": "shape", "definition": tag}]}), (mode, eo, pts.tolist())


def rand_layered_translucent_scene(rng):
    """2-6 random polygons of alpha 255 ... 1 over each other in a 150x90 frame."""
    import scenarios
    W, H = 150, 90
    kids = []
    for _ in range(int(rng.integers(2, 7))):
        n = int(rng.integers(3, 8))
        pts = rng.uniform(-10, 1, (n, 2)) * 0 + rng.uniform(0, 1, (n, 2)) * [W, H]
        col = scenarios._rgba(*[int(v) for v in rng.integers(0, 256, 3)], int(rng.choice([255, 200, 128, 31, 1])))
        kids.append({"type": "shape", "definition": scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": col})})
    return dict(width=W, height=H, stage={"children": kids})


def rand_stroked_scene(rng):
    """1-3 random stroked (morph) shapes in a 120x100 frame: curves, rectilinear box strokes, round caps / joins, hairlines,
    reflected and off-frame placements."""
    import scenarios
    from test_host import _rand_path_shape
    W, H = 120, 100
    kids = []
    for _ in range(int(rng.integers(1, 4))):
        morph = bool(rng.integers(0, 3) == 0)
        tag = _rand_path_shape(rng, int(rng.choice([1, 2, 5, 20, 45, 90, 200])), morph)
        sx, sy = float(rng.choice([1, 1, 0.6, 1.7, -1])), float(rng.choice([1, 1, 0.8, 1.3]))
        mat = scenarios._m(sx, sy, int(rng.integers(-300, 900)) + (2000 if sx < 0 else 0), int(rng.integers(-300, 500)),
                           float(rng.choice([0, 0, 0.2])), float(rng.choice([0, 0, -0.15])))
        kids.append({"type": "morph-shape", "definition": tag, "ratio": float(rng.uniform(0, 1)), "matrix": mat} if morph else
                    {"type": "shape", "definition": tag, "matrix": mat})
    return dict(width=W, height=H, stage={"children": kids})


def comb_shape(teeth, width_twips):
    """One path of `teeth` narrow teeth over a bar: 2 * teeth edges active in most rows."""
    import scenarios
    pts = []
    step = width_twips / teeth
    for k in range(teeth):
        pts += [(100 + step * k, 100), (100 + step * k + step / 2, 1900)]
    pts += [(100 + width_twips + 100, 1950), (50, 1950)]
    return scenarios._poly_shape(pts, {"type": "solid", "color": scenarios._rgba(1, 2, 3)})


def crowded_rows_scene(teeth, even_odd):
    """The frame of test_crowded_rows_vs_oracle: a comb of `teeth` teeth (24 ... 6000 active edges per row)."""
    tag = comb_shape(teeth, 2000 if teeth <= 140 else 6000)
    return dict(width=120 if teeth <= 140 else 320, height=100, even_odd=even_odd, stage={"children": [{"type": "shape", "definition": tag}]})


def comb_points(teeth, width_twips, x0, y_top, y_bottom):
    pts = []
    step = width_twips / teeth
    for k in range(teeth):
        pts += [(x0 + step * k, y_top), (x0 + step * k + step / 2, y_bottom)]
    pts += [(x0 + width_twips + 100, y_bottom + 50), (x0 - 50, y_bottom + 50)]
    return pts


def frame_top_scene(teeth, y_top, even_odd):
    """The frame of test_edges_arriving_together_at_the_frame_top_vs_oracle: 2 * teeth edges of one translucent path that become
    active together at sample row 0 (the frame's top edge clips them)."""
    import scenarios
    tag = scenarios._poly_shape(comb_points(teeth, 2200, 60, y_top, 1700), {"type": "solid", "color": scenarios._rgba(200, 30, 90, 180)})
    return dict(width=128, height=96, even_odd=even_odd, stage={"children": [{"type": "shape", "definition": tag}]})


def uncovered_path_row_scenes():
    """The frames of test_tile_with_an_uncovered_path_row_is_not_a_full_cover: a triangle whose last pixel row has no active sample
    row, opaque and translucent, at three bottoms; then the two soak scenes that found it.  [(key, scene)]"""
    import scenarios
    out = []
    for sy in (1.0001, 1.0, 1.002):                                  # bottom at y = 242.026 (the case), 242.0, 242.48
        pts = np.array([(9.75, 213.40), (350.65, 242.0), (155.5, 242.0)])
        for col in (scenarios._rgba(200, 80, 40, 255), scenarios._rgba(200, 80, 40, 140)):
            tag = scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": col})
            out.append(((sy, col["a"]), dict(width=512, height=300, stage={"children": [{"type": "shape", "definition": tag, "matrix": scenarios._m(1.0, sy)}]})))
    for case in (("big", 200, 551), ("big", 200, 572)):
        out.append((case, soak_scene(*case)))
    return out


def wide_frame_parts():
    """Shapes of test_frames_wider_than_a_cell_column_field (a 9600x48 frame): a translucent triangle beyond column 9000 (`far`), an
    opaque one near the left (`near`), a solid path wider than 8192 px opaque and translucent (`wide`, `wide_t`), a shallow sliver
    crossing a block boundary inside an anti-aliased span, and the wide path with a radial gradient (`wide_grad`)."""
    import scenarios
    far = scenarios._poly_shape([(9000 * 20 + 7, 100), (9500 * 20 + 3, 300), (9200 * 20, 900)], {"type": "solid", "color": scenarios._rgba(200, 100, 50, 160)})
    near = scenarios._poly_shape([(50, 60), (4000, 130), (900, 880)], {"type": "solid", "color": scenarios._rgba(20, 200, 50)})
    pts = [(100, 100), (9400 * 20, 200), (9400 * 20, 700), (100, 600), (3000 * 20, 350)]
    wide = scenarios._poly_shape(pts, {"type": "solid", "color": scenarios._rgba(1, 2, 3)})
    wide_t = scenarios._poly_shape(pts, {"type": "solid", "color": scenarios._rgba(200, 30, 90, 140)})
    # a shallow edge crossing column 5 + 8192 (the block boundary of a path that starts at x = 5) inside an anti-aliased span
    sliver = scenarios._poly_shape([(100, 400), (9590 * 20, 470), (9590 * 20, 520), (100, 430)], {"type": "solid", "color": scenarios._rgba(10, 90, 250, 200)})
    grad = {"type": "radial-gradient", "matrix": scenarios._m(4.0, 0.02, 4800 * 20, 400),
            "gradient": scenarios._grad([(0, (255, 0, 0)), (128, (0, 255, 0, 90)), (255, (0, 0, 255))])}
    return dict(far=far, near=near, wide=wide, wide_t=wide_t, sliver=sliver, wide_grad=scenarios._poly_shape(pts, grad))


WIDE_FRAME = (9600, 48)


def wide_frame_scenes():
    """Every frame of test_frames_wider_than_a_cell_column_field: {key: scene}."""
    w, h = WIDE_FRAME
    p = wide_frame_parts()
    combos = {"near_far": ["near", "far"], "wide": ["wide"], "near_wide_t_far": ["near", "wide_t", "far"],
              "wide_sliver_wide_t": ["wide", "sliver", "wide_t"], "wide_sliver": ["wide", "sliver"], "near_wide_grad": ["near", "wide_grad"]}
    return {k: dict(width=w, height=h, stage={"children": [{"type": "shape", "definition": p[n]} for n in v]}) for k, v in combos.items()}


# ---- raw edge lists (Renderer.render_edges / the oracle's swfo_fill_edges)
RAW_LIMIT = 1 << 23                     # +-32768 px in 24.8


def random_raw_pair(rng, W, H):
    """Two random lines anywhere in +-2^23 active over the same [top, bottom) with opposite directions (the edges active in a row
    then balance, as the edges of a closed polygon do): top / bottom inside both lines, now and then strictly inside them; half of
    the lines have an end point near the frame.  Now and then both are never active (top == bottom)."""
    L = RAW_LIMIT
    top, bottom = sorted(int(v) for v in rng.integers(-L, L + 1, 2))
    if rng.integers(0, 2):
        top, bottom = sorted(int(v) for v in rng.integers(-2 * H * 256, 3 * H * 256, 2))
    if top == bottom:
        bottom += 1
    out = []
    for d in (1, -1):
        y1 = top if rng.integers(0, 2) else int(rng.integers(-L, top + 1))
        y2 = bottom if rng.integers(0, 2) else int(rng.integers(bottom, L + 1))
        near = rng.integers(0, 2)
        x1 = int(rng.integers(-2 * W * 256, 3 * W * 256)) if near else int(rng.integers(-L, L + 1))
        x2 = int(rng.integers(-L, L + 1))
        out.append((x1, y1, x2, y2, top, bottom, d))
    if rng.integers(0, 6) == 0:                       # never active, both
        out = [(x1, y1, x2, y2, t, t, d) for x1, y1, x2, y2, t, b, d in out]
    return out


def rand_raw_frame(rng, it):
    """One frame of the raw-edge fuzz: (W, H, groups), 1-3 paths of random edge pairs, both fill rules, opaque and translucent."""
    W, H = [(64, 48), (333, 97), (97, 333)][it % 3]
    groups = []
    for _ in range(int(rng.integers(1, 4))):
        edges = []
        for _ in range(int(rng.integers(1, 12))):
            edges += random_raw_pair(rng, W, H)
        argb = int(rng.choice([0xff000000 | int(rng.integers(0, 1 << 24)), 0x80402010, 0x20101000]))
        groups.append((edges, bool(rng.integers(0, 2)), argb))
    return W, H, groups


def raw_scene(W, H, groups):
    """groups: [(edge rows (x1, y1, x2, y2, top, bottom, dir), even_odd, premultiplied ARGB)], one path each with the frame as its
    rectangle, painted in order.  Returns (edges, paths, styles) for Renderer.render_edges."""
    from swf_renderer_amd import api
    rows, paths, styles = [], np.zeros(len(groups), api.PATH_DTYPE), []
    clear = True
    for i, (edges, eo, argb) in enumerate(groups):
        e = np.zeros(len(edges), api.EDGE_DTYPE)
        for k, name in enumerate(("x1", "y1", "x2", "y2", "top", "bottom", "dir")):
            e[name] = [r[k] for r in edges]
        e["reserved"] = i
        paths[i] = (sum(len(r) for r in rows), len(e), api.PATH_TOR, int(eo), i, int((argb >> 24) == 255 or clear), 0, 0, W, H)
        rows.append(e)
        styles.append(api.solid_style(argb))
        clear = False
    return np.concatenate(rows), paths, styles


def raw_oracle(W, H, groups):
    """The oracle's frame of raw_scene(W, H, groups)."""
    edges, _, _ = raw_scene(W, H, groups)
    be = ob.OracleBackend(W, H)
    at = 0
    for edge_rows, eo, argb in groups:
        be.fill_edges(edges[at:at + len(edge_rows)], (0, 0, W, H), eo, argb)
        at += len(edge_rows)
    want = be.premultiplied_rgba()
    be.close()
    return want


def raw_product(W, H, groups):
    import swf_renderer_amd as S
    r = S.Renderer(W, H)
    try:
        r.render_edges(*raw_scene(W, H, groups))
        return r.read_image(premultiplied=True)
    finally:
        r.close()


# ---- dense mixed-fill frames: every kind of path and style layered deep enough that the strips of the shaded tile instances see
#      dozens of entries (staging rounds, the StripTop cull, cell fetches beyond 16 per row, box paths, the compacted edge-pixel blend)
def _dense_gradient(rng, W, H, kind):
    import scenarios
    n = int(rng.integers(1, 9))
    ratios = sorted(int(v) for v in rng.integers(0, 256, n))
    if n > 2 and rng.integers(0, 3) == 0:
        ratios[1] = ratios[0]
    colors = [(ratios[i], (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.choice([255, 255, 128, 0, 37]))))
              for i in range(n)]
    # the gradient circle is at least 0.6 frame diagonals wide and centred in the frame: every sample stays within two radii
    ky = float(rng.uniform(0.5, 1.0))
    sc = float(rng.uniform(0.6, 3.0)) * 20 / 16384 * float(np.hypot(W, H)) / ky
    t = float(rng.uniform(-3.2, 3.2))
    c, sn = np.cos(t), np.sin(t)
    fill = {"type": kind, "gradient": scenarios._grad(colors),
            "matrix": scenarios._m(sc * c, sc * ky * c, int(rng.integers(0, W * 20)), int(rng.integers(0, H * 20)), sc * sn, -sc * ky * sn)}
    if kind == "focal-gradient":
        fill["focal_point"] = {"epsilons": int(rng.integers(-240, 241))}
    return fill


def _dense_bitmap(rng, W, H, bitmap_id, magnified):
    import scenarios
    k = float(rng.uniform(1.6, 9.0)) if magnified else float(rng.uniform(0.15, 0.7))
    t = float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 2) else 0.0
    c, sn = np.cos(t), np.sin(t)
    return {"type": "bitmap", "bitmap_id": bitmap_id, "repeating": bool(rng.integers(0, 2)), "smoothed": True,
            "matrix": scenarios._m(20 * k * c, 20 * k * c, int(rng.integers(-200, W * 20)), int(rng.integers(-200, H * 20)), 20 * k * sn, -20 * k * sn)}


DENSE_KINDS = ("solid", "rect_fill", "rect_stroke", "bitmap_mag", "bitmap_min", "radial", "focal", "stroke", "linear")


def rand_dense_scene(rng, linear=False, width=None, height=None, shapes=None):
    """One frame of many layered shapes of every kind -- opaque and translucent solids (alpha 1 ... 254), rectilinear fills and strokes
    (box paths), repeating and clamped bitmap fills magnified (bilinear, also across the texture's border) and minified (convolution),
    radial and focal gradients, strokes of polygons -- with opaque covers of the whole frame in the middle of the stack (the StripTop
    cull), a translucent first shape on the clear surface (the lerp route), a width that is not a multiple of 64 and a tile-row count
    that is not a multiple of 8.  linear=True adds ONE shape with a linear gradient (the +-1 LSB extension: two of them overlapping
    could differ by 2)."""
    import scenarios
    if width is None:
        W = int(rng.integers(2, 5)) * 64 + int(rng.integers(1, 64))
    else:
        W = width
    if height is None:
        tile_rows = int(rng.choice([3, 4, 5, 6, 7]))
        H = (tile_rows - 1) * 16 + int(rng.integers(1, 17))
    else:
        H = height
    bitmaps = [make_bitmap_tag(3, int(rng.integers(2, 12)), int(rng.integers(2, 12)), rng),
               make_bitmap_tag(4, int(rng.integers(24, 64)), int(rng.integers(24, 64)), rng)]
    kinds = [k for k in DENSE_KINDS if k != "linear"]
    n = shapes if shapes is not None else int(rng.integers(45, 70))
    cover_at = sorted(int(v) for v in rng.choice(np.arange(n // 3, 2 * n // 3), 2, replace=False))
    linear_at = int(rng.integers(cover_at[1] + 1, n)) if linear else -1
    kids = []

    def shape(tag, mat=None):
        kids.append({"type": "shape", "definition": tag} if mat is None else {"type": "shape", "definition": tag, "matrix": mat})

    def polygon(big):
        m = int(rng.integers(3, 8))
        if big:
            return rng.uniform(-0.15, 1.15, (m, 2)) * [W, H]
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(6, 0.5 * max(W, H))
        a = np.sort(rng.uniform(0, 2 * np.pi, m))
        return np.stack([cx + r * np.cos(a), cy + r * rng.uniform(0.3, 1.0) * np.sin(a)], -1)

    def color(alpha=None):
        a = alpha if alpha is not None else int(rng.choice([255, 255, int(rng.integers(1, 255)), int(rng.integers(1, 255)), 1, 254]))
        return scenarios._rgba(*[int(v) for v in rng.integers(0, 256, 3)], a)

    # the first shape lands on the clear surface: translucent (SOURCE-lerp)
    shape(scenarios._poly_shape(np.rint(polygon(True) * 20), {"type": "solid", "color": color(int(rng.integers(1, 255)))}))
    for i in range(n):
        if i in cover_at:
            # an opaque cover of the whole frame: a rectangle (box path) or a polygon reaching past every side (tor path)
            if i == cover_at[0]:
                pts = np.array([(-1.5, -2.25), (W + 3.0, -2.25), (W + 3.0, H + 1.75), (-1.5, H + 1.75)])
            else:
                pts = np.array([(-0.4 * W, -0.3 * H), (1.7 * W, -0.2 * H), (0.5 * W, 2.2 * H)])
            shape(scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": color(255)}))
            continue
        kind = "linear" if i == linear_at else kinds[int(rng.integers(0, len(kinds)))]
        big = bool(rng.integers(0, 3))
        if kind == "solid":
            shape(scenarios._poly_shape(np.rint(polygon(big) * 20), {"type": "solid", "color": color()}))
        elif kind in ("rect_fill", "rect_stroke"):
            x0, y0 = rng.uniform(-0.1 * W, 0.8 * W), rng.uniform(-0.1 * H, 0.8 * H)
            x1, y1 = x0 + rng.uniform(2, W), y0 + rng.uniform(2, H)
            q = (lambda v: float(np.round(v))) if rng.integers(0, 2) else (lambda v: float(v))       # on pixel edges or anywhere
            pts = np.array([(q(x0), q(y0)), (q(x1), q(y0)), (q(x1), q(y1)), (q(x0), q(y1))])
            mat = scenarios._m(float(rng.choice([1, 1, 0.75, 1.5])), float(rng.choice([1, 1, 1.25])))
            if kind == "rect_fill":
                shape(scenarios._poly_shape(np.rint(pts / [mat["scale_x"] / 65536, mat["scale_y"] / 65536] * 20), {"type": "solid", "color": color()}), mat)
            else:
                shape(scenarios._poly_shape(np.rint(pts * 20), None, line=color(), line_width=int(rng.choice([20, 30, 50, 90, 170]))))
        elif kind in ("bitmap_mag", "bitmap_min"):
            mag = kind == "bitmap_mag"
            fill = _dense_bitmap(rng, W, H, 3 if mag else 4, mag)
            shape(scenarios._poly_shape(np.rint(polygon(big) * 20), fill))
        elif kind in ("radial", "focal", "linear"):
            fill = _dense_gradient(rng, W, H, {"radial": "radial-gradient", "focal": "focal-gradient", "linear": "linear-gradient"}[kind])
            shape(scenarios._poly_shape(np.rint(polygon(big) * 20), fill))
        else:                                   # a stroked polygon, sometimes filled too (two paths)
            fill = {"type": "solid", "color": color()} if rng.integers(0, 2) else None
            shape(scenarios._poly_shape(np.rint(polygon(big) * 20), fill, line=color(), line_width=int(rng.choice([10, 25, 60, 140]))))
    return dict(width=W, height=H, bitmaps=bitmaps, stage={"children": kids})


def strip_path_counts(width, height, paths):
    """Paths whose pixel rectangle meets each 64x8 strip of a frame: an int array of (tile-rows * 2, tile columns)."""
    sw, sh = (width + 63) // 64, (height + 7) // 8
    cnt = np.zeros((sh, sw), int)
    for p in paths:
        if p["x_max"] <= p["x_min"] or p["y_max"] <= p["y_min"]:
            continue
        cnt[p["y_min"] // 8:(p["y_max"] - 1) // 8 + 1, p["x_min"] // 64:(p["x_max"] - 1) // 64 + 1] += 1
    return cnt


# ---- gradient edges: focal points on and beyond the circle (|focal| >= 1: the a == 0 branch of the walker, cones with transparent
#      regions), and 1, 2 and SWFR_MAX_STOPS stops
GRADIENT_EDGE_FOCALS = (256, -256, 257, -257, 384, -384, 1024, -1024, 32767, -32768)     # Sfixed8P8 epsilons: +-1, +-1.004, ..., 128, -128


def gradient_edge_stops(n, rng):
    """n stops with translucent colours; from 4 stops on, duplicate ratios (a hard step) and a transparent stop."""
    ratios = sorted(int(v) for v in rng.integers(0, 256, n))
    if n >= 4:
        ratios[2] = ratios[1]
        ratios[-1] = ratios[-2]
    alphas = [255, 128, 37, 0, 200, 255]
    return [(ratios[i], (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), alphas[(i * 5 + n) % len(alphas)])) for i in range(n)]


def gradient_edge_scenes():
    """{key: scene}: a focal gradient for every epsilon of GRADIENT_EDGE_FOCALS with 1, 2 and 16 stops, on a clear frame and over an
    opaque backdrop, plus a radial gradient with 16 stops.  The gradient circle is centred in the frame and at least as large as the
    frame's diagonal, and the shape lies inside the frame: every sample stays within one radius of the centre (pixman's 16.16 range
    is never left)."""
    import scenarios
    W, H = 90, 70
    out = {}
    rng = np.random.default_rng(1616)
    back = scenarios._poly_shape([(-100, -60), (W * 20 + 80, 40), (W * 20 + 40, H * 20 + 90), (60, H * 20 + 50)], {"type": "solid", "color": scenarios._rgba(30, 90, 160)})
    shape_pts = np.array(scenarios._circleish(W * 10, H * 10, 0.46 * H * 20, 20)) * [W / H, 1.0] + [-(W / H - 1) * W * 10, 0]
    cases = [(f, n) for f in GRADIENT_EDGE_FOCALS for n in (1, 2, 16)] + [(None, 16)]
    for i, (focal, n) in enumerate(cases):
        r = float(np.hypot(W, H)) * (1.0 + 0.15 * (i % 3))              # radius in pixels
        sc = r * 20 / 16384
        t = 0.37 * i
        c, sn = np.cos(t), np.sin(t)
        fill = {"type": "radial-gradient" if focal is None else "focal-gradient", "gradient": scenarios._grad(gradient_edge_stops(n, rng)),
                "matrix": scenarios._m(sc * c, sc * c, W * 10 + i % 5, H * 10 - i % 7, sc * sn, -sc * sn)}
        if focal is not None:
            fill["focal_point"] = {"epsilons": focal}
        for backdrop in (False, True):
            kids = ([{"type": "shape", "definition": back}] if backdrop else []) + [{"type": "shape", "definition": scenarios._poly_shape(np.rint(shape_pts), fill)}]
            out["%s_%d_%s" % ("radial" if focal is None else "focal%d" % focal, n, "over" if backdrop else "clear")] = dict(width=W, height=H, stage={"children": kids})
    return out


# ---- a batch corpus: frames of one size, one kind of frame per code path a group of swfr_render_batch frames can mix
#      (tests/test_gpu_batches.py; tests/test_host.py checks that every kind keeps what it is in the corpus for)
BATCH_W, BATCH_H = 160, 120
BATCH_TIE_CASE = ("mixed", 2000, 1265)            # a SOAK_TIE_CASES scene whose tied rows lie inside BATCH_W x BATCH_H


def _placed(stage, sx, sy, tx, ty):
    """a stage's objects inside one container placed by scale (sx, sy) and translation (tx, ty) twips"""
    import scenarios
    return {"type": "container", "matrix": scenarios._m(sx, sy, tx, ty), "children": stage["children"]}


def batch_corpus(W=BATCH_W, H=BATCH_H):
    """{kind: scene} re-framed to W x H: the empty stage; box paths only; solid polygons only (the compact style table); a translucent
    stack; bitmap fills (magnified, minified, repeat, no-repeat); radial and focal gradients; a linear gradient (the +-1 LSB
    extension); round-joined strokes (queued rows); a soak scene with tied edges (the list-order replay); a crowded comb (k2_rows_huge);
    one path of more than ROWS_STAGE edges; a colour-transformed bitmap scene (the texel pass); morph shapes at several ratios.
    Every scene's bitmaps use the ids of tests/scenarios.py's fixture bitmap (3) only."""
    import scenarios
    SC = scenarios.scenarios()
    rgba = scenarios._rgba

    def poly(pts_px, fill, line=None, line_width=0):
        return {"type": "shape", "definition": scenarios._poly_shape(np.rint(np.asarray(pts_px, float) * 20), fill, line=line, line_width=line_width)}

    def rect(x0, y0, x1, y1):
        return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]

    out = {"empty": {"children": []}}
    out["boxes"] = {"children": [
        poly(rect(8, 6, 60, 40), {"type": "solid", "color": rgba(200, 40, 30)}),                        # whole pixels
        poly(rect(30.35, 22.6, 97.15, 71.05), {"type": "solid", "color": rgba(20, 90, 220, 140)}),      # fractional
        poly(rect(101.5, 9.25, 155.75, 30.5), {"type": "solid", "color": rgba(250, 250, 20, 255)}),
        poly(rect(70, 50, 150, 110), None, line=rgba(10, 140, 60, 200), line_width=50),                   # rectilinear strokes
        poly(rect(12.3, 60.45, 55.1, 113.7), None, line=rgba(0, 0, 0), line_width=23)]}
    out["solid"] = {"children": [
        poly([(5, 3), (150, 20), (90, 115)], {"type": "solid", "color": rgba(30, 160, 220)}),
        poly([(120, 5), (158, 60), (130, 117), (60, 100), (70, 40)], {"type": "solid", "color": rgba(230, 120, 10, 200)}),
        poly([(-20, 70), (80, 50), (40, 140)], {"type": "solid", "color": rgba(90, 20, 120, 37)})]}
    out["translucent"] = SC["translucent_stack"]["stage"]
    out["bitmaps"] = {"children": SC["bitmap_no_repeat_magnified"]["stage"]["children"] + SC["bitmap_no_repeat_minified"]["stage"]["children"][:1] +
                      SC["bitmap_repeat_over_solid"]["stage"]["children"][1:] + SC["bitmap_minified_rotated"]["stage"]["children"]}
    out["radial_focal"] = {"children": [_placed(SC["gradient_radial"]["stage"], 0.7, 0.7, 0, 0),
                                        _placed(SC["gradient_focal"]["stage"], 0.8, 0.7, 1300, 700),
                                        _placed(SC["gradient_alpha_over"]["stage"], 0.5, 0.5, 1500, 0)]}
    out["linear"] = SC["gradient_linear_ext"]["stage"]
    out["round_strokes"] = SC["morph_round_stroke_090"]["stage"]
    out["tie"] = soak_scene(*BATCH_TIE_CASE)["stage"]
    out["comb"] = crowded_rows_scene(60, False)["stage"]
    out["long_path"] = {"children": [poly(scenarios._circleish(80, 60, 55, n=50), {"type": "solid", "color": rgba(40, 200, 120, 180)}),
                                     poly([(10, 10), (50, 12), (30, 40)], {"type": "solid", "color": rgba(200, 0, 0)})]}
    ct = {"red_mult": {"epsilons": 256}, "green_mult": {"epsilons": 160}, "blue_mult": {"epsilons": 90}, "alpha_mult": {"epsilons": 220},
          "red_add": 20, "green_add": -10, "blue_add": 40, "alpha_add": 0}
    out["cxform"] = {"children": [{"type": "container", "color_transform": ct, "children": SC["bitmap_minified_rotated"]["stage"]["children"]}]}
    out["morph"] = {"children": [_placed(SC["morph_000"]["stage"], 0.55, 0.55, 0, 0), _placed(SC["morph_128"]["stage"], 0.55, 0.6, 1500, 100),
                                 _placed(SC["morph_color_030"]["stage"], 0.6, 0.55, 300, 1150), _placed(SC["morph_255"]["stage"], 0.5, 0.5, 1700, 1300)]}
    bitmaps = SC["bitmap_minified_rotated"]["bitmaps"]
    return {k: dict(width=W, height=H, stage=st, bitmaps=bitmaps if k in ("bitmaps", "cxform") else []) for k, st in out.items()}
