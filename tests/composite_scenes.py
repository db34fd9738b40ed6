"""Random frames for the blend and layer instances of the tile kernel, checked against tests/frame_model.py.

- rand_composited_scene: display trees of solid polygons, rectilinear fills and strokes and stroked polygons (the solid kinds of
  helpers.rand_dense_scene) wrapped at random in "blend_mode" containers, colour transforms and "layer" objects nested up to four deep,
  with the cases the clear-surface bookkeeping and the culling have to get right.
- RawFrame and the raw_* corpora: frames written directly as swfr_upload_edges arrays, aimed at the walk of k2_tiles<3|4> over one
  strip's list: groups whose BEGIN, first member and END fall on either side of the staging rounds (16 entries), the class-byte chunks
  (64) and the prefetched class bytes (128); nesting with the first path of a strip at every level; opaque covers around groups.
- shaded=True gives the trees bitmap and radial / focal leaves; a RawFrame path may carry a bitmap or radial style of its own
  (bitmap_style, radial_style), and SHADED_CLASSES / shaded_frames aim one such member at each branch of the bitmap fetch of the tile
  pass, in every setting a member can stand in (tests/test_shaded_composite_fuzz_gpu.py); shaded_reach counts, from the sample positions
  of tests/pad_model.py, which branch each wavefront takes.
- strip_lists / strip_reach: what a frame's strips see, from the arrays alone (by path rectangle, as helpers.strip_path_counts), so
  that a test can show that its frames reach the positions it is about.
"""
import numpy as np

import blend_model as bm
import layer_model as lm
import mask_model as mk
import scenarios

MODES = ["normal"] + sorted(bm.MODES)                 # the nine operators, by the names "blend_mode" / "layer" take
BEGIN, END, MASK = lm.PATH_GROUP_BEGIN, lm.PATH_GROUP_END, mk.PATH_GROUP_MASK
STRIP_W, STRIP_H, TILE_H = 64, 8, 16
ROUND, CHUNK, PREFETCH = 16, 64, 128                  # k2_tiles: entries staged per round, class bytes per chunk, class bytes fetched up front


# ---------------------------------------------------------------------------------------------------------------- display trees
def _cxform(rng):
    mult = [int(v) for v in rng.choice([256, 256, 200, 128, 96, 384], 4)]
    add = [int(v) for v in rng.choice([0, 0, 0, 20, -30, 60], 4)]
    d = {}
    for c, m, a in zip(("red", "green", "blue", "alpha"), mult, add):
        d[c + "_mult"] = {"epsilons": m}
        d[c + "_add"] = a
    return d


SHADED_BITMAP_SIZES = ((1, 1), (1, 6), (5, 1), (2, 2), (3, 3), (3, 5), (7, 5), (7, 7), (47, 48))      # (width, height)
SPREAD_NAMES = ("pad", "reflect", "repeat")


def rand_texels(rng, bw, bh, opaque=False):
    """(bh, bw, 4) straight RGBA bytes: a third of the texels translucent, some of those alpha 0 (as pad_scenes.random_box_case's)"""
    px = rng.integers(0, 256, (bh, bw, 4)).astype(np.uint8)
    if opaque:
        px[..., 3] = 255
    else:
        px[..., 3] = np.where(rng.integers(0, 3, (bh, bw)) == 0, np.where(rng.integers(0, 4, (bh, bw)) == 0, 0, px[..., 3]), 255)
    return px


def _shaded_leaf(rng, W, H, bitmaps, shape, polygon):
    """a shape with a bitmap fill (all three edge rules, magnified and minified, rotated and mirrored, often at negative offsets) or a
    radial / focal gradient with one of the three spreads, the polygon within reach of pixman's 16.16 positions"""
    if rng.integers(0, 2):
        bid = int(rng.choice(sorted(bitmaps)))
        bw, bh = bitmaps[bid][:2]
        if rng.integers(0, 3) == 0:
            kx, ky = float(rng.uniform(0.3, 0.74)), float(rng.uniform(0.3, 3.0))                # minified: the convolution
            if rng.integers(0, 2):
                kx, ky = ky, kx
        else:
            kx, ky = float(rng.uniform(0.76, 12.0)), float(rng.uniform(0.76, 12.0))
        if bw > 16:
            kx, ky = min(kx, 3.0), min(ky, 3.0)
        t = float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 3) == 0 else 0.0
        c, s = np.cos(t), np.sin(t)
        if rng.integers(0, 4) == 0:
            kx = -kx                                                                          # mirrored
        extend = ("none", "repeat", "pad")[int(rng.integers(0, 3))]
        matrix = scenarios._m(20 * kx * c, 20 * ky * c, int(rng.integers(-W * 6, W * 20)), int(rng.integers(-H * 6, H * 20)), 20 * kx * s, -20 * ky * s)
        fill = {"type": "bitmap", "bitmap_id": bid, "repeating": extend == "repeat", "smoothed": True, "matrix": matrix}
        if extend == "pad":
            fill["pad"] = True
        if rng.integers(0, 3) == 0:
            x0, y0 = float(rng.integers(-4, W - 8)), float(rng.integers(-4, H - 4))
            x1, y1 = x0 + float(rng.integers(8, W)), y0 + float(rng.integers(3, H))
            pts = np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
        else:
            pts = polygon(bool(rng.integers(0, 2)))
        return shape(scenarios._poly_shape(np.rint(pts * 20), fill))
    focal = bool(rng.integers(0, 2))
    radius = float(rng.uniform(6, 0.45 * max(W, H)))
    cx, cy = float(rng.uniform(0, W)), float(rng.uniform(0, H))
    n = int(rng.integers(1, 6))
    ratios = sorted(int(v) for v in rng.integers(0, 256, n))
    if n > 2 and rng.integers(0, 3) == 0:
        ratios[1] = ratios[0]
    colors = [(ratios[i], (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.choice([255, 255, 128, 0, 37])))) for i in range(n)]
    t = float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 2) else 0.0
    c, s = np.cos(t), np.sin(t)
    k = radius * 20 / 16384.0
    fill = {"type": "focal-gradient" if focal else "radial-gradient", "gradient": dict(scenarios._grad(colors), spread=SPREAD_NAMES[int(rng.integers(0, 3))]),
            "matrix": scenarios._m(k * c, k * c, round(cx * 20), round(cy * 20), k * s, -k * s)}
    if focal:
        fill["focal_point"] = {"epsilons": int(rng.integers(-200, 201))}
    reach = (0.8 if focal else 1.25) * radius                        # (rotated: within two radii of the centre and of the focus on both axes)
    m = int(rng.integers(3, 7))
    pts = np.stack([cx + rng.uniform(-reach, reach, m), cy + rng.uniform(-reach, reach, m)], -1)
    return shape(scenarios._poly_shape(np.rint(pts * 20), fill))


def _without_transforms_around_bitmaps(obj):
    """the tree with "color_transform" taken off every object that holds a bitmap fill: a recoloured bitmap is a variant texture of the
    handle that walked the stage, which neither tests/frame_model.py nor another handle can be given"""
    def holds(o):
        if isinstance(o, dict):
            return (o.get("type") == "bitmap" and "bitmap_id" in o) or any(holds(v) for v in o.values())
        return isinstance(o, list) and any(holds(v) for v in o)
    if isinstance(obj, list):
        return [_without_transforms_around_bitmaps(o) for o in obj]
    if isinstance(obj, dict):
        return {k: _without_transforms_around_bitmaps(v) for k, v in obj.items() if not (k == "color_transform" and holds(obj))}
    return obj


def rand_composited_scene(rng, width=None, height=None, min_children=0, leaves=None, shaded=False):
    """One frame: a random tree over about `leaves` shapes.  Always present: a translucent first path on the clear surface (sometimes
    inside a layer), an empty layer, layers wholly and partly off the frame, clear sources (alpha 0, plain and under an operator),
    opaque covers of the whole frame below, between, inside and above layers, colour-transform wrappers, all nine operators on layers
    and "blend_mode" containers, layers nested up to four deep.  The width is no multiple of 64 (often none of 4), the height no
    multiple of 16 (often none of 8).  min_children: at least so many children of the stage (a threaded build cuts pieces of 64).
    shaded: two leaves in five are bitmap fills (texels registered as straight RGBA, sc["raw_bitmaps"]) and radial / focal gradients
    (_shaded_leaf); off, every seed draws what it always drew."""
    W = width if width is not None else int(rng.integers(1, 4)) * 64 + int(rng.integers(1, 64))
    H = height if height is not None else int(rng.integers(1, 5)) * 16 + int(rng.integers(1, 16))
    rgba = scenarios._rgba
    raw_bitmaps = {}
    if shaded:
        for k, i in enumerate(rng.choice(len(SHADED_BITMAP_SIZES), 4, replace=False)):
            bw, bh = SHADED_BITMAP_SIZES[int(i)]
            raw_bitmaps[21 + k] = (bw, bh, rand_texels(rng, bw, bh, opaque=k == 0).tobytes())

    def color(alpha=None):
        a = alpha if alpha is not None else int(rng.choice([255, 255, int(rng.integers(1, 255)), int(rng.integers(1, 255)), 1, 254, 0]))
        return rgba(*[int(v) for v in rng.integers(0, 256, 3)], a)

    def polygon(big):
        m = int(rng.integers(3, 8))
        if big:
            return rng.uniform(-0.15, 1.15, (m, 2)) * [W, H]
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 0.4 * max(W, H))
        a = np.sort(rng.uniform(0, 2 * np.pi, m))
        return np.stack([cx + r * np.cos(a), cy + r * rng.uniform(0.3, 1.0) * np.sin(a)], -1)

    def shape(tag, mat=None):
        return {"type": "shape", "definition": tag} if mat is None else {"type": "shape", "definition": tag, "matrix": mat}

    def cover():
        if rng.integers(0, 2):                          # a rectangle (box path) or a polygon reaching past every side (tor path)
            pts = np.array([(-1.5, -2.25), (W + 3.0, -2.25), (W + 3.0, H + 1.75), (-1.5, H + 1.75)])
        else:
            pts = np.array([(-0.4 * W, -0.3 * H), (1.7 * W, -0.2 * H), (0.5 * W, 2.2 * H)])
        return shape(scenarios._poly_shape(np.rint(pts * 20), {"type": "solid", "color": color(255)}))

    def leaf():
        if shaded and rng.integers(0, 5) < 2:
            return _shaded_leaf(rng, W, H, raw_bitmaps, shape, polygon)
        kind = ("solid", "rect_fill", "rect_stroke", "stroke")[int(rng.integers(0, 4))]
        big = bool(rng.integers(0, 3) == 0)
        if kind == "solid":
            return shape(scenarios._poly_shape(np.rint(polygon(big) * 20), {"type": "solid", "color": color()}))
        if kind in ("rect_fill", "rect_stroke"):
            x0, y0 = rng.uniform(-0.1 * W, 0.8 * W), rng.uniform(-0.1 * H, 0.8 * H)
            x1, y1 = x0 + rng.uniform(2, W), y0 + rng.uniform(2, H)
            q = (lambda v: float(np.round(v))) if rng.integers(0, 2) else (lambda v: float(v))
            pts = np.array([(q(x0), q(y0)), (q(x1), q(y0)), (q(x1), q(y1)), (q(x0), q(y1))])
            if kind == "rect_fill":
                mat = scenarios._m(float(rng.choice([1, 1, 0.75, 1.5])), float(rng.choice([1, 1, 1.25])))
                return shape(scenarios._poly_shape(np.rint(pts / [mat["scale_x"] / 65536, mat["scale_y"] / 65536] * 20), {"type": "solid", "color": color()}), mat)
            return shape(scenarios._poly_shape(np.rint(pts * 20), None, line=color(), line_width=int(rng.choice([20, 30, 50, 90]))))
        fill = {"type": "solid", "color": color()} if rng.integers(0, 2) else None
        return shape(scenarios._poly_shape(np.rint(polygon(big) * 20), fill, line=color(), line_width=int(rng.choice([10, 25, 60]))))

    budget = [leaves if leaves is not None else int(rng.integers(12, 40))]

    def layer(depth, kids=None, **kw):
        obj = {"type": "container", "layer": MODES[int(rng.integers(0, 9))], "children": members(depth + 1) if kids is None else kids, **kw}
        if rng.integers(0, 4) == 0:
            obj["blend_mode"] = MODES[int(rng.integers(0, 9))]
        if rng.integers(0, 5) == 0:
            obj["color_transform"] = _cxform(rng)
        return obj

    def members(depth):
        """the children of a container at layer depth `depth`"""
        out = []
        for _ in range(int(rng.integers(1, 6))):
            if budget[0] <= 0:
                break
            r = int(rng.integers(0, 20))
            if r < 9:
                budget[0] -= 1
                k = leaf()
                if r == 0:
                    k["blend_mode"] = MODES[int(rng.integers(0, 9))]
                if r == 1 and depth < lm.MAX_DEPTH:
                    k["layer"] = MODES[int(rng.integers(0, 9))]             # a shape that is a layer itself
                out.append(k)
            elif r < 14 and depth < lm.MAX_DEPTH:
                out.append(layer(depth))
            elif r < 16:
                out.append({"type": "container", "blend_mode": MODES[int(rng.integers(0, 9))], "children": members(depth)})
            elif r < 18:
                out.append({"type": "container", "color_transform": _cxform(rng), "children": members(depth)})
            elif r == 18:
                budget[0] -= 1
                out.append(cover())
            elif depth < lm.MAX_DEPTH:
                out.append(layer(depth, kids=[]))                           # an empty group
        return out

    def nest(depth):
        """layers nested `depth` deep around one shape, shapes before and after at every level"""
        kids = [leaf()]
        for _ in range(depth):
            kids = ([leaf()] if rng.integers(0, 2) else []) + [layer(0, kids=kids)] + ([leaf()] if rng.integers(0, 2) else [])
        return kids

    first = shape(scenarios._poly_shape(np.rint(polygon(True) * 20), {"type": "solid", "color": color(int(rng.integers(1, 255)))}))
    lead = []
    for _ in range(int(rng.integers(0, 3))):            # what may come first and leave the surface clear, or not
        r = int(rng.integers(0, 4))
        lead.append([layer(0, kids=[]),
                     layer(0, kids=[leaf()], matrix=scenarios._m(1, 1, (W + 50) * 20, 0)),
                     shape(scenarios._poly_shape(np.rint(polygon(True) * 20), {"type": "solid", "color": color(0)})),
                     dict(shape(scenarios._poly_shape(np.rint(polygon(True) * 20), {"type": "solid", "color": color(0)})), blend_mode=MODES[int(rng.integers(0, 9))])][r])
    kids = lead + [layer(0, kids=[first]) if rng.integers(0, 3) == 0 else first]
    kids += members(0)
    kids += [cover(), layer(0)]                                             # a cover directly below a layer
    kids += [cover(), layer(0, kids=[leaf(), cover(), leaf()])]             # between two layers; inside one
    kids += [layer(0, kids=[]), layer(0, kids=[leaf(), leaf()], matrix=scenarios._m(1, 1, -(W + 60) * 20, (H + 40) * 20))]   # empty; wholly off the frame
    kids += [layer(0, kids=[leaf(), leaf()], matrix=scenarios._m(1, 1, int(rng.integers(W * 8, W * 14)), int(rng.integers(-H * 10, H * 10))))]   # partly off
    kids += nest(int(rng.integers(2, lm.MAX_DEPTH + 1)))
    while budget[0] > 0:
        kids += members(0)
    if rng.integers(0, 2):
        kids += [layer(0), cover()]                                         # a cover directly above a layer
    kids += members(0) if rng.integers(0, 2) else []
    while len(kids) < min_children:
        budget[0] = 8
        kids += members(0)
    if shaded:
        return dict(width=W, height=H, raw_bitmaps=raw_bitmaps, stage={"children": _without_transforms_around_bitmaps(kids)})
    return dict(width=W, height=H, stage={"children": kids})


def cairo_render_shaded(sc, aliased=False):
    """premultiplied RGBA of a shaded tree through libcairo: the canvas replay of the fade scenes over a CairoBackend whose surface
    patterns take CAIRO_EXTEND_PAD where the fill says "pad" and whose gradients take their fill's spread"""
    import ctypes

    import blend_scenes as bs
    import fade_scenes as fs
    import mask_scenes as ms
    import pad_scenes as ps
    import spread_scenes as ss
    from oracle import cairo_backend as cb

    class Backend(cb.CairoBackend):
        surface_extend, gradient_extend = None, ss.CAIRO_EXTEND["pad"]

        def set_fill_pattern(self, bitmap, repeat):
            super().set_fill_pattern(bitmap, repeat)
            if self.surface_extend is not None:
                self._fill = self._fill[:2] + (self.surface_extend,)

        def set_fill_radial(self, *a):
            super().set_fill_radial(*a)
            self.lib.cairo_pattern_set_extend(self._fill[1], self.gradient_extend)

    class Replay(fs.FadeReplay):
        def _draw_path(self, path):
            fill = path.get("fill", {})
            self.be.surface_extend = ps.CAIRO_EXTEND["pad"] if fill.get("repeating") == "pad" else None
            self.be.gradient_extend = ss.CAIRO_EXTEND[(fill.get("gradient") or {}).get("spread", "pad")]
            return super()._draw_path(path)

    be = Backend(sc["width"], sc["height"])
    try:
        if aliased:
            f = be.lib.cairo_set_antialias
            f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
            f(be.cr, bs.CAIRO_ANTIALIAS_NONE)
        low = ms._lowering(sc.get("bitmaps", []))
        stage = low.lower(ps.for_cairo(sc["stage"]))
        rp = Replay(be, linear_extension=True)
        for bid, (w, h, px) in list(low.extra.items()) + list(sc.get("raw_bitmaps", {}).items()):
            rp.bitmaps[bid] = be.create_bitmap(w, h, px)
        rp.render(stage)
        return be.premultiplied_rgba().copy()
    finally:
        be.close()


# ---------------------------------------------------------------------------------------------------------------- raw frames
class RawFrame:
    """A frame in swfr_upload_edges form (include/swfr.h), written path by path.  Coordinates are pixels (floats are rounded to 24.8);
    colours premultiplied ARGB words; `op` an operator name of MODES.  A path's rectangle is its extents cut to the frame; a group's
    markers get the union of the rectangles of the paths between them when the group is closed.  A group is begin(); paths; end(op),
    or, masked, begin(); content; mask(); mask paths; end(op); end(op, opacity) puts the fade 255 - opacity into bits 24..31 of the
    END's lerp."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.rows, self.paths, self.pixels, self.open = [], [], [], []
        self.masks = []                                              # per open group: the index of its MASK marker, or None
        self.bitmaps = {}                                            # id -> (width, height, straight RGBA bytes): what the bitmap styles name

    @staticmethod
    def _fx(v):
        return int(round(float(v) * 256))

    def _rect(self, xs, ys):
        x0, x1 = max(min(xs) >> 8, 0), min((max(xs) + 255) >> 8, self.W)
        y0, y1 = max(min(ys) >> 8, 0), min((max(ys) + 255) >> 8, self.H)
        if x0 >= x1 or y0 >= y1:                                     # off the frame: an empty rectangle inside it
            x0 = x1 = min(max(x0, 0), self.W)
            y0 = y1 = min(max(y0, 0), self.H)
        return x0, y0, x1, y1

    def _path(self, kind, rows, rect, argb, lerp, op, even_odd=False, style=None):
        """style: for a bitmap or radial path, rect -> its api.Style (one style per path: it belongs to the path's rectangle)"""
        assert not (lerp and op != "normal")
        first = len(self.rows)
        self.rows += rows
        field = int(lerp) | (bm.OPERATORS["over" if op == "normal" else op] << 8)
        self.paths.append([first, len(rows), kind, int(even_odd), len(self.pixels), field, *rect])
        self.pixels.append(style(rect) if style is not None else argb & 0xffffffff)
        return self

    def tor(self, pts, argb, lerp=0, op="normal", even_odd=False, style=None):
        p = [(self._fx(x), self._fx(y)) for x, y in pts]
        rows = []
        for a, b in zip(p, p[1:] + p[:1]):
            if a[1] < b[1]:
                rows.append((a[0], a[1], b[0], b[1], a[1], b[1], 1, 0))
            elif a[1] > b[1]:
                rows.append((b[0], b[1], a[0], a[1], b[1], a[1], -1, 0))
        return self._path(0, rows, self._rect([q[0] for q in p], [q[1] for q in p]), argb, lerp, op, even_odd, style)

    def rect_tor(self, x0, y0, x1, y1, argb, lerp=0, op="normal", style=None):
        return self.tor([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], argb, lerp, op, style=style)

    def box(self, x0, y0, x1, y1, argb, lerp=0, op="normal", style=None):
        """a box path of one box, cut to the frame (a box lies inside its path's rectangle)"""
        a = [max(self._fx(x0), 0), max(self._fx(y0), 0), min(self._fx(x1), self.W * 256), min(self._fx(y1), self.H * 256)]
        if a[0] >= a[2] or a[1] >= a[3]:
            return self._path(1, [], self._rect([a[0]], [a[1]])[:2] * 2, argb, lerp, op, style=style)
        return self._path(1, [(a[0], a[1], a[2], a[3], a[1], a[3], 1, 0)], self._rect([a[0], a[2]], [a[1], a[3]]), argb, lerp, op, style=style)

    def begin(self):
        self.open.append(len(self.paths))
        self.masks.append(None)
        self.paths.append([len(self.rows), 0, BEGIN, 0, 0, 0, 0, 0, 0, 0])
        return self

    def mask(self):
        assert self.masks and self.masks[-1] is None
        self.masks[-1] = len(self.paths)
        self.paths.append([len(self.rows), 0, MASK, 0, 0, 0, 0, 0, 0, 0])
        return self

    def end(self, op="normal", opacity=255):
        b, m = self.open.pop(), self.masks.pop()
        rects = [p[6:10] for p in self.paths[b + 1:] if p[6] < p[8] and p[7] < p[9]]
        rect = [min(r[0] for r in rects), min(r[1] for r in rects), max(r[2] for r in rects), max(r[3] for r in rects)] if rects else [0, 0, 0, 0]
        self.paths[b][6:10] = rect
        inner = 0                                                    # (an empty member, or a group that is empty as a whole, of a placed
        for p in self.paths[b + 1:]:                                 #  group: an empty rectangle inside the group's)
            empty = not (p[6] < p[8] and p[7] < p[9])
            if empty and (inner == 0 or moving):
                p[6:10] = [rect[0], rect[1], rect[0], rect[1]]
            if p[2] == BEGIN:
                if inner == 0:
                    moving = empty
                inner += 1
            elif p[2] == END:
                inner -= 1
        if m is not None:
            self.paths[m][6:10] = rect
        self.paths.append([len(self.rows), 0, END, 0, 0, bm.OPERATORS["over" if op == "normal" else op] << 8 | (255 - int(opacity)) << 24, *rect])
        return self

    @property
    def depth(self):
        return len(self.open)

    @property
    def levels(self):
        """the levels of SWFR_MAX_LAYER_DEPTH the open groups take: two for one that holds a MASK"""
        return sum(2 if m is not None else 1 for m in self.masks)

    def arrays(self):
        from swf_renderer_amd import api
        assert not self.open
        e = np.zeros(len(self.rows), api.EDGE_DTYPE)
        for k, name in enumerate(("x1", "y1", "x2", "y2", "top", "bottom", "dir", "reserved")):
            e[name] = [r[k] for r in self.rows]
        p = np.zeros(len(self.paths), api.PATH_DTYPE)
        for i, row in enumerate(self.paths):
            p[i] = tuple(row)
        return e, p, [px if isinstance(px, api.Style) else api.solid_style(px) for px in self.pixels]

    def add_bitmap(self, texels):
        """registers (h, w, 4) straight RGBA texels with the frame; the id a bitmap style names"""
        bid = 31 + len(self.bitmaps)
        self.bitmaps[bid] = (texels.shape[1], texels.shape[0], np.ascontiguousarray(texels, np.uint8).tobytes())
        return bid

    def model_bitmaps(self):
        """the frame's bitmaps as tests/frame_model.py takes them: {id: (h, w) premultiplied 0xAARRGGBB}"""
        import pad_model as pm
        return {bid: pm.premultiply(np.frombuffer(px, np.uint8).reshape(h, w, 4)) for bid, (w, h, px) in self.bitmaps.items()}


def without_markers(edges, paths, styles):
    """the same frame with its group markers removed: every path composited on its own (the blend instance)"""
    return edges, paths[paths["kind"] < BEGIN], styles


def premultiplied(rng, alpha=None):
    a = int(alpha if alpha is not None else rng.choice([255, int(rng.integers(1, 255)), int(rng.integers(1, 255)), 1, 254, 0]))
    r, g, b = (int(v) * a // 255 for v in rng.integers(0, 256, 3))
    return (a << 24) | (r << 16) | (g << 8) | b


MEMBER_CLASSES = ("full_opaque", "full_translucent", "full_lerp", "full_lerp_opaque", "box", "partial")


def add_member(fr, rng, cls, op, x0, y0, first=False):
    """One path of class `cls` whose rectangle reaches the strip at (x0, y0) (the strip's corner, pixels): a full cover of some of the
    strip's rows over the whole tile width (opaque or translucent; with the lerp bit clear under `op`, or set), a box, or a triangle.
    `first`: the first paint of a group (its surface is clear: a plain path has the lerp bit set there)."""
    ya = y0 + int(rng.integers(0, 6))
    yb = ya + int(rng.integers(1, 4))
    lerp = 1 if (first and op in ("normal", "add")) else 0
    if lerp:
        op = "normal"
    if cls.startswith("full"):
        opaque = cls in ("full_opaque", "full_lerp_opaque")
        if cls.startswith("full_lerp"):
            lerp, op = 1, "normal"
        # (whole pixel rows, reaching past the tile on both sides where the frame does: a full cover of the rows in this tile)
        fr.rect_tor(x0 - int(rng.integers(0, 3)), ya, x0 + STRIP_W + int(rng.integers(0, 9)), yb, premultiplied(rng, 255 if opaque else int(rng.integers(1, 255))), lerp, op)
    elif cls == "box":
        xa = x0 + float(rng.uniform(0, 50))
        q = (lambda v: float(np.round(v))) if rng.integers(0, 2) else (lambda v: v)
        fr.box(q(xa), q(ya + float(rng.uniform(0, 1))), q(xa + float(rng.uniform(2, 40))), q(yb + float(rng.uniform(0.6, 2))), premultiplied(rng), lerp, op)
    else:
        xa = x0 + float(rng.uniform(0, 56))
        fr.tor([(xa, ya + float(rng.uniform(0, 1))), (xa + float(rng.uniform(3, 50)), ya + float(rng.uniform(0, 3))), (xa + float(rng.uniform(-4, 20)), yb + float(rng.uniform(1, 5)))],
               premultiplied(rng), lerp, op)


def raw_group_sizes_frame(rng, n_members, n_before, n_after=3, W=70, H=13, end_op=None):
    """`n_before` plain entries, ONE group of `n_members` members, `n_after` plain entries, every one of them reaching the strip in the
    frame's top left corner (so that a list position in that strip is the count of the paths before it): BEGIN sits at position
    n_before, the first member behind it, END at n_before + n_members + 1.  Classes and operators go round with the member's index,
    from a random start."""
    fr = RawFrame(W, H)
    c0, o0 = int(rng.integers(0, 6)), int(rng.integers(0, 9))
    for i in range(n_before):
        add_member(fr, rng, ("full_translucent", "box", "partial")[i % 3], MODES[(o0 + i) % 9] if i else "normal", 0, 0, first=i == 0)
    fr.begin()
    for i in range(n_members):
        add_member(fr, rng, MEMBER_CLASSES[(c0 + i) % 6], MODES[(o0 + i) % 9], 0, 0, first=i == 0)
    fr.end(end_op or MODES[(o0 + n_members) % 9])
    for i in range(n_after):
        add_member(fr, rng, ("partial", "full_translucent", "box")[i % 3], MODES[(o0 + 2 * i) % 9], 0, 0)
    return fr


def rand_raw_nested_frame(rng, W=200, H=45, items=60, member_size=(3, 40), cover_chance=0.04, spread=None):
    """Random nesting, one to four deep, of small members scattered over a frame of several tile rows and columns: in one strip the
    first path to arrive may sit at any level (levels above it are set aside together, or never), a group may reach a strip by its
    markers' rectangle alone, siblings reuse a stack level, and different strips of the frame take different branches.  Opaque covers
    of the whole frame (lerp bit set, tor or box) appear at any depth.  spread: the members of an outermost group lie within so many
    pixels of one point (a large frame: the group's rectangle, which the model composites, stays small)."""
    fr = RawFrame(W, H)
    anchor = [0.0, 0.0]
    painted = [False]                                                # per open surface: has it been painted (the lerp rule's "still clear")

    def member():
        s = float(rng.uniform(*member_size))
        x, y = float(rng.uniform(-5, W)), float(rng.uniform(-5, H))
        if spread is not None and fr.depth:
            x, y = anchor[0] + float(rng.uniform(0, spread)), anchor[1] + float(rng.uniform(0, spread))
        r = float(rng.random())
        op = MODES[int(rng.integers(0, 9))] if rng.integers(0, 2) else "normal"
        first = not painted[-1]
        if r < cover_chance and (spread is None or not fr.depth):
            if rng.integers(0, 2):
                fr.rect_tor(-2, -2, W + 2, H + 2, premultiplied(rng, 255), 1)
            else:
                fr.box(0, 0, W, H, premultiplied(rng, 255), 1)
        elif r < 0.4:
            add_member(fr, rng, MEMBER_CLASSES[int(rng.integers(0, 4))], op, (int(x) // 64) * 64 if x >= 0 else 0, (int(max(y, 0)) // 8) * 8, first=first)
        elif r < 0.65:
            lerp = 1 if first and op in ("normal", "add") else 0
            fr.box(x, y, x + s, y + float(rng.uniform(1, 20)), premultiplied(rng), lerp, "normal" if lerp else op)
        else:
            lerp = 1 if first and op in ("normal", "add") else 0
            pts = [(x + float(rng.uniform(0, s)), y + float(rng.uniform(0, s * 0.6))) for _ in range(int(rng.integers(3, 6)))]
            fr.tor(pts, premultiplied(rng), lerp, "normal" if lerp else op, even_odd=bool(rng.integers(0, 2)))
        painted[-1] = True

    n = 0
    while n < items or fr.depth:
        r = float(rng.random())
        if n >= items:
            r = 0.95                                                 # close what is open
        if r < 0.55:
            member()
            n += 1
        elif r < 0.8 and fr.depth < lm.MAX_DEPTH:
            if not fr.depth:
                anchor[:] = [float(rng.uniform(-5, W)), float(rng.uniform(-5, H))]
            fr.begin()
            painted.append(False)
            n += 1
        elif fr.depth:
            fr.end(MODES[int(rng.integers(0, 9))])
            painted.pop()
            painted[-1] = True                                       # (a composite counts as a paint: what follows is OVER)
        else:
            member()
            n += 1
    return fr


def raw_nesting_frame(first_level, depth, W=200, H=45, seed=0):
    """Groups nested `depth` deep in which the first path to reach strip column 0 sits at level `first_level` (1..depth): the levels
    above it have members only in the tile columns further right, those below only behind it.  Then a sibling group at level 1 (the
    stack level reused), a group that reaches the first strips by its rectangle alone between two that paint there, and plain paths."""
    rng = np.random.default_rng(seed * 100 + first_level * 10 + depth)
    fr = RawFrame(W, H)
    add_member(fr, rng, "partial", "normal", 0, 0, first=True)
    fr.rect_tor(0, 2, W, 5, premultiplied(rng, 120))
    for lvl in range(1, depth + 1):
        fr.begin()
        if lvl < first_level:
            add_member(fr, rng, "partial", "normal", 128, 16, first=True)          # elsewhere: tile column 2, the second tile row
        else:
            add_member(fr, rng, MEMBER_CLASSES[(lvl + first_level) % 6], MODES[(lvl * 2 + first_level) % 9], 0, 0, first=lvl == first_level)
            add_member(fr, rng, "box", MODES[(lvl + 3) % 9], 64, 8)
    for lvl in range(depth, 0, -1):
        if lvl >= first_level:
            add_member(fr, rng, "partial", MODES[(lvl + 5) % 9], 0, 0)
        fr.end(MODES[(lvl * 3 + first_level + depth) % 9])
        add_member(fr, rng, "full_translucent", MODES[(lvl + 1) % 9], 0, 0)
    fr.begin()                                                        # a sibling: level 1 again
    add_member(fr, rng, "full_translucent", "normal", 0, 0, first=True)
    add_member(fr, rng, "partial", "multiply", 0, 0)
    fr.end("difference")
    fr.begin()                                                        # present in the first strips by its rectangle only
    add_member(fr, rng, "box", "normal", 0, 32, first=True)
    add_member(fr, rng, "box", "screen", 128, 0)
    fr.end("multiply")
    fr.begin()
    add_member(fr, rng, "partial", "normal", 0, 0, first=True)
    fr.end("hardlight")
    add_member(fr, rng, "partial", "overlay", 0, 0)
    return fr


COVER_PLACES = ("below_begin", "between_siblings", "above_end", "last", "inside", "inside_nested")


def raw_cover_frame(place, kind, W=130, H=37, seed=0):
    """Two sibling groups (the second nested two deep) over a translucent ground, and ONE opaque cover of the whole frame with the lerp
    bit set (`kind`: "tor" or "box") at `place`: where the walk of a strip may start behind it, and where it must not."""
    rng = np.random.default_rng(seed + 17 * COVER_PLACES.index(place) + (kind == "box"))
    fr = RawFrame(W, H)

    def cover():
        if kind == "tor":
            fr.rect_tor(-3, -3, W + 3, H + 3, premultiplied(rng, 255), 1)
        else:
            fr.box(0, 0, W, H, premultiplied(rng, 255), 1)

    def scatter(n, first=False):
        for i in range(n):
            add_member(fr, rng, MEMBER_CLASSES[int(rng.integers(0, 6))] if not (first and i == 0) else "partial", MODES[int(rng.integers(0, 9))],
                       64 * int(rng.integers(0, (W + 63) // 64)), 8 * int(rng.integers(0, (H + 7) // 8)), first=first and i == 0)

    fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 150), 1)
    scatter(4)
    if place == "below_begin":
        cover()
    fr.begin()
    scatter(5, first=True)
    if place == "inside":
        cover()
        scatter(3)
    fr.end(MODES[int(rng.integers(1, 9))])
    if place == "between_siblings":
        cover()
    fr.begin()
    scatter(3, first=True)
    fr.begin()
    scatter(3, first=True)
    if place == "inside_nested":
        cover()
        scatter(2)
    fr.end(MODES[int(rng.integers(1, 9))])
    scatter(2)
    fr.end(MODES[int(rng.integers(1, 9))])
    if place == "above_end":
        cover()
    scatter(4)
    if place == "last":
        cover()
    return fr


def raw_many_groups_frame(rng, W=1000, H=520, groups=3000):
    """several thousand small groups of one to three members, now and then one inside another, plain paths between them"""
    fr = RawFrame(W, H)
    fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, 200), 1)
    for g in range(groups):
        x, y = float(rng.uniform(-4, W - 4)), float(rng.uniform(-4, H - 4))
        nested = g % 7 == 0
        fr.begin()
        for i in range(int(rng.integers(1, 4))):
            op = MODES[int(rng.integers(0, 9))]
            lerp = 1 if i == 0 and op in ("normal", "add") else 0
            if i == 1 and nested:
                fr.begin()
                fr.box(x + 1, y + 2, x + 9.5, y + 7.25, premultiplied(rng), 1)
                fr.end(MODES[int(rng.integers(0, 9))])
            if rng.integers(0, 3):
                fr.tor([(x + float(rng.uniform(0, 12)), y + float(rng.uniform(0, 12))) for _ in range(3)], premultiplied(rng), lerp, "normal" if lerp else op)
            else:
                fr.box(x, y, x + float(rng.uniform(1, 14)), y + float(rng.uniform(1, 14)), premultiplied(rng), lerp, "normal" if lerp else op)
        fr.end(MODES[g % 9])
        if g % 5 == 0:
            fr.tor([(x + float(rng.uniform(0, 30)), y + float(rng.uniform(0, 30))) for _ in range(3)], premultiplied(rng), 0, MODES[int(rng.integers(0, 9))])
    return fr


# ---------------------------------------------------------------------------------------------------------------- what the strips see
def strip_lists(width, height, paths):
    """{(strip row, tile column): [path index, ...]}: the paths whose pixel rectangle meets each 64x8 strip, in painter's order"""
    out = {}
    for i, p in enumerate(paths):
        if p["x_max"] <= p["x_min"] or p["y_max"] <= p["y_min"]:
            continue
        for sy in range(int(p["y_min"]) // STRIP_H, (int(p["y_max"]) - 1) // STRIP_H + 1):
            for sx in range(int(p["x_min"]) // STRIP_W, (int(p["x_max"]) - 1) // STRIP_W + 1):
                out.setdefault((sy, sx), []).append(i)
    return out


def band_positions(height, paths):
    """{tile row: {path index: its position among the paths whose rectangle meets the tile row}}: where a path's class byte sits in
    the 64-entry chunks of a strip of that tile row"""
    out = {}
    for i, p in enumerate(paths):
        if p["x_max"] <= p["x_min"] or p["y_max"] <= p["y_min"]:
            continue
        for t in range(int(p["y_min"]) // TILE_H, (int(p["y_max"]) - 1) // TILE_H + 1):
            d = out.setdefault(t, {})
            d[i] = len(d)
    return out


def strip_reach(width, height, paths):
    """What the walk of each strip meets, from the arrays alone.  Returns a dict:
    in_group      the most entries between an outermost BEGIN and its END in one strip (the markers not counted)
    markers       [(kind, position in the strip's list, position in its tile row's list)] of every marker in every strip
    first_levels  the set of levels (1..4) at which the first non-marker path of an outermost group arrived in some strip
    bare_ends     the set of depths d at which an END closed a group no path of which (nor of a group inside it) reached the strip
    together      the most open levels whose first path in a strip was one and the same path
    sibling_reuse whether some strip saw two groups at one level inside one parent, both with paths there
    marker_only_between  whether some strip saw a group without paths there between two outermost groups with paths there"""
    bands = band_positions(height, paths)
    in_group, markers, first_levels, bare_ends, together = 0, [], set(), set(), 0
    sibling_reuse = marker_only_between = False
    for (sy, sx), lst in strip_lists(width, height, paths).items():
        band = bands[sy * STRIP_H // TILE_H]
        start, reached = 0, []                                       # reached[d]: a path has reached the strip since the open group of level d + 1 began
        top_history = []                                             # the strip's outermost groups: did a path reach the strip inside them
        for pos, i in enumerate(lst):
            kind = int(paths[i]["kind"])
            if kind == BEGIN:
                markers.append((BEGIN, pos, band[i]))
                if not reached:
                    start = pos
                reached.append(False)
            elif kind == END:
                markers.append((END, pos, band[i]))
                if not reached.pop():
                    bare_ends.add(len(reached) + 1)
                if not reached:
                    in_group = max(in_group, pos - start - 1)
                    top_history.append(any(int(paths[j]["kind"]) < BEGIN for j in lst[start:pos]))
                    if top_history[-3:] == [True, False, True]:
                        marker_only_between = True
                    if top_history[-2:] == [True, True]:
                        sibling_reuse = True
            elif reached:
                if not any(reached):
                    first_levels.add(len(reached))
                together = max(together, reached.count(False))
                reached[:] = [True] * len(reached)
    return dict(in_group=in_group, markers=markers, first_levels=first_levels, bare_ends=bare_ends, together=together,
                sibling_reuse=sibling_reuse, marker_only_between=marker_only_between)


# ---------------------------------------------------------------------------------------------------------------- the raw corpus
GROUP_SIZES = (14, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128, 129, 200)
BEFORE = tuple(range(18))                             # plain entries before BEGIN
BEFORE_LONG = (62, 63, 64, 65, 126, 127, 128, 129)    # ... of a short group: BEGIN itself at the chunk boundaries
EDGE_SIZES = ((70, 13), (61, 20), (130, 37), (203, 45), (64, 8), (66, 17))       # widths % 4, % 64 and heights % 8, % 16 of every kind
NESTINGS = [(first, depth) for depth in range(1, 5) for first in range(1, depth + 1)]
NESTED_SEEDS = 40


def group_size_frames(n):
    """(k, frame) for the group size n and every count k of plain entries before its BEGIN; the frame sizes go round"""
    for k in BEFORE:
        W, H = ((70, 13), (64, 16), (61, 9), (130, 12))[(n + k) % 4]
        yield k, raw_group_sizes_frame(np.random.default_rng(6000 + 100 * n + k), n, k, n_after=3 + k % 3, W=W, H=H)


def late_group_frames():
    """(k, frame): a short group behind k plain entries, k around a class-byte chunk and the prefetched class bytes"""
    for k in BEFORE_LONG:
        yield k, raw_group_sizes_frame(np.random.default_rng(6300 + k), 5 + k % 3, k, W=(70, 64)[k % 2], H=(13, 16)[k % 2])


def nested_frames(count=NESTED_SEEDS):
    """(seed, frame): random nesting over the frame sizes of EDGE_SIZES"""
    for seed in range(count):
        W, H = EDGE_SIZES[seed % len(EDGE_SIZES)]
        yield seed, rand_raw_nested_frame(np.random.default_rng(6700 + seed), W=W, H=H, items=int(30 + 17 * (seed % 5)))


def raw_corpus_reach():
    """What the strips of the raw corpus (every group size, every k, every nesting, every seed) see, from the arrays alone: strip_reach
    summed up, plus `operator_positions`, the list positions of the paths with an operator in the frames without their markers"""
    out = dict(in_group=0, markers=[], first_levels=set(), bare_ends=set(), together=0, sibling_reuse=False, marker_only_between=False,
               operator_positions=set())
    frames = [fr for n in GROUP_SIZES for _, fr in group_size_frames(n)] + [fr for _, fr in late_group_frames()]
    frames += [raw_nesting_frame(f, d) for f, d in NESTINGS] + [fr for _, fr in nested_frames()]
    for fr in frames:
        _, paths, _ = fr.arrays()
        rc = strip_reach(fr.W, fr.H, paths)
        out["in_group"] = max(out["in_group"], rc["in_group"])
        out["together"] = max(out["together"], rc["together"])
        out["markers"] += rc["markers"]
        out["first_levels"] |= rc["first_levels"]
        out["bare_ends"] |= rc["bare_ends"]
        out["sibling_reuse"] |= rc["sibling_reuse"]
        out["marker_only_between"] |= rc["marker_only_between"]
        plain = paths[paths["kind"] < BEGIN]
        for lst in strip_lists(fr.W, fr.H, plain).values():
            out["operator_positions"] |= {pos for pos, i in enumerate(lst) if int(plain[i]["lerp"]) >> 8}
    return out


def assert_reach(rc):
    """the conditions under which the raw corpus tests what it claims to (conditions, not tolerances)"""
    assert rc["in_group"] > PREFETCH > CHUNK > ROUND, rc["in_group"]      # a group of more than 128 (so of more than 64, and 16) entries in one strip
    for kind in (BEGIN, END):
        for which in (1, 2):                                          # position in the strip's own list, and in its tile row's list
            pos = {m[which] for m in rc["markers"] if m[0] == kind}
            for edge in (ROUND, CHUNK, PREFETCH):                     # the marker as the last entry before the boundary and the first behind it
                assert edge - 1 in pos and edge in pos, (kind, which, edge)
    assert rc["first_levels"] == {1, 2, 3, 4}, rc["first_levels"]     # a strip's first path at every level
    assert rc["bare_ends"] >= {1, 2, 3, 4}, rc["bare_ends"]           # ENDs of groups never set aside, at every depth
    assert rc["together"] == lm.MAX_DEPTH                             # four levels set aside by one path
    assert rc["sibling_reuse"] and rc["marker_only_between"]
    for edge in (ROUND, CHUNK, PREFETCH):                             # the blend instance: operators on both sides of the boundaries
        assert {edge - 1, edge, edge + 1} <= rc["operator_positions"], edge


# ---------------------------------------------------------------------------------------------------------------- shaded members
# (tests/test_shaded_composite_fuzz_gpu.py)  Each class is aimed at one branch of the bitmap fetch of the tile pass; which branch a
# strip takes is worked out from the positions of tests/pad_model.py (strip_halves), and the matrices are drawn until it is the one.
SHADED_CLASSES = ("bitmap_inside_plain", "bitmap_inside_translucent", "bitmap_inside_partial", "bitmap_rim_none", "bitmap_rim_repeat",
                  "bitmap_rim_pad", "bitmap_minified", "radial_spread")
RAW_BITMAP_SIZES = ((1, 1), (1, 5), (2, 2), (3, 3), (5, 3), (7, 7), (47, 48))          # (width, height)
GRADIENT_R = 16384.0


def bitmap_style(bid, extend, kx, ky, ox, oy, t=0.0):
    """the api.Style of bitmap `bid` drawn with texels of kx x ky pixels (negative: mirrored), turned by t, the bitmap's corner at pixel
    (ox, oy); `inv` is Cairo's pattern matrix, the inverse of that placement"""
    import spread_model as sm
    from swf_renderer_amd import api
    c, s = float(np.cos(t)), float(np.sin(t))
    st = api.Style()
    st.kind, st.bitmap, st.extend = api.STYLE_BITMAP, bid, extend
    st.inv[:] = sm.invert((kx * c, kx * s, -ky * s, ky * c, float(ox), float(oy)))
    return st


def radial_style(extend, radius, cx, cy, stops, focal=0.0, t=0.0):
    """the api.Style of a radial (focal: a focal) gradient of `radius` pixels around pixel (cx, cy), as the frame builder writes it: the
    circles (focal R, 0, 0) -> (0, 0, R) with R = 16384.  stops: [(ratio 0..255, (r, g, b, a) bytes, straight)]"""
    import spread_model as sm
    from swf_renderer_amd import api
    c, s = float(np.cos(t)), float(np.sin(t))
    k = radius / GRADIENT_R
    st = api.Style()
    st.kind, st.extend = api.STYLE_RADIAL, extend
    st.inv[:] = sm.invert((k * c, k * s, -k * s, k * c, float(cx), float(cy)))
    st.c0x, st.c0y, st.r0, st.c1x, st.c1y, st.r1 = focal * GRADIENT_R, 0.0, 0.0, 0.0, 0.0, GRADIENT_R
    st.n_stops = len(stops)
    for i, (ratio, rgba) in enumerate(stops):
        st.stop_offset[i] = ratio / 255.0
        for ch in range(4):
            st.stop_rgba[i][ch] = rgba[ch] / 255.0
    return st


def strip_halves(st, rect, bw, bh, sx, sy):
    """What the two row halves (four rows by 64 columns each: one wavefront's 256 samples) of the strip at (sx, sy) see of a bitmap
    style whose path has the rectangle rect, from the sample positions of tests/pad_model.py: [(bilinear, inside)] -- whether the filter
    is the bilinear one and whether every one of the 256 samples has its four taps strictly inside the bitmap"""
    import pad_model as pm
    import spread_model as sm
    inv = tuple(float(v) for v in st.inv)
    bilinear = pm.filter_of(inv) is None
    (bx, by), ((m00, m01), (m10, m11)) = sm.to_pixman(inv, rect)
    out = []
    for h in (0, 1):
        px, py = np.meshgrid(np.arange(sx, sx + STRIP_W, dtype=np.int64), np.arange(sy + 4 * h, sy + 4 * h + 4, dtype=np.int64))
        tx, ty = (bx + px * m00 + py * m01 - 0x8000) >> 16, (by + px * m10 + py * m11 - 0x8000) >> 16
        out.append((bilinear, bool(((tx >= 0) & (tx <= bw - 2) & (ty >= 0) & (ty <= bh - 2)).all())))
    return out


def _covered_halves(rect, y0):
    """the row halves of the strip at row y0 that the rectangle's rows meet"""
    return [h for h in (0, 1) if rect[1] < y0 + 4 * h + 4 and rect[3] > y0 + 4 * h]


def add_shaded_member(fr, rng, cls, op, x0, y0, lerp=0):
    """One path of class `cls` of SHADED_CLASSES in the strip at (x0, y0), under `op` or with the lerp bit.

    bitmap_inside_plain        whole pixel rows of whole row halves right across the strip, an opaque bitmap so far magnified that every
                               tap of the half lies inside it: the `inside` fetch and the `plain` copy
    bitmap_inside_translucent  the same, texels translucent and alpha 0 among them: `inside`, arithmetic
    bitmap_inside_partial      a triangle or a box off the pixel grid over such a strip: `inside`, coverage below 255 and lanes without any
    bitmap_rim_none/repeat/pad the bitmap's edge runs through the strip (1 x 1, 1 x n and 2 x 2 bitmaps, rotated and mirrored, corners at
                               negative positions): the general fetch with its outside flags, wrap and clamp
    bitmap_minified            a scale below 0.75 on an axis: the convolution, the edge rule going round
    radial_spread              a radial or focal gradient, reflected, repeated or padded"""
    assert cls in SHADED_CLASSES and not (lerp and op != "normal")
    whole = cls in ("bitmap_inside_plain", "bitmap_inside_translucent") or (cls != "bitmap_inside_partial" and rng.integers(0, 2))
    if whole:
        h0, h1 = [(0, 1), (1, 2), (0, 2)][int(rng.integers(0, 3))]
        geometry = ("rect", (x0 - int(rng.integers(0, 3)), y0 + 4 * h0, x0 + STRIP_W + int(rng.integers(0, 9)), y0 + 4 * h1))
    elif rng.integers(0, 2):
        xa, ya = x0 + float(rng.uniform(0, 40)), y0 + float(rng.uniform(0, 5))
        geometry = ("box", (xa, ya, xa + float(rng.uniform(2, 40)), ya + float(rng.uniform(1.5, 6))))
    else:
        xa, ya = x0 + float(rng.uniform(0, 50)), y0 + float(rng.uniform(0, 4))
        geometry = ("tor", [(xa, ya), (xa + float(rng.uniform(3, 50)), ya + float(rng.uniform(0, 3))), (xa + float(rng.uniform(-4, 20)), ya + float(rng.uniform(2, 8)))])

    def bitmap(rect):
        inside = cls.startswith("bitmap_inside")
        sizes = [s for s in RAW_BITMAP_SIZES if not inside or min(s) > 1]
        halves = _covered_halves(rect, y0) or [0]
        for _ in range(400):
            bw, bh = sizes[int(rng.integers(0, len(sizes)))]
            if inside:
                kx, ky = 64.0 / (bw - 1) * float(rng.uniform(1.1, 2.5)), max(0.8, 4.0 / (bh - 1) * float(rng.uniform(1.1, 4.0)))
                t = float(rng.uniform(-0.02, 0.02)) if rng.integers(0, 3) == 0 else 0.0
                u, v = float(rng.uniform(0.6, max(0.7, bw - 0.6 - 64.0 / kx))), float(rng.uniform(0.6, max(0.7, bh - 0.6 - 8.0 / ky)))
                ox, oy = x0 + 0.5 - kx * u, y0 + 0.5 - ky * v
                if rng.integers(0, 4) == 0:                          # mirrored: the strip's right edge at u
                    kx, ox = -kx, x0 + 63.5 + kx * u
                extend = int(rng.integers(0, 3))
            else:
                if cls == "bitmap_minified":
                    kx, ky = float(rng.uniform(0.3, 0.74)), float(rng.uniform(0.3, 3.0))
                    if rng.integers(0, 2):
                        kx, ky = ky, kx
                    extend = int(rng.integers(0, 3))
                else:
                    kx, ky = float(rng.uniform(0.76, 12.0)), float(rng.uniform(0.76, 12.0))
                    extend = {"bitmap_rim_none": 0, "bitmap_rim_repeat": 1, "bitmap_rim_pad": 2}[cls]
                t = float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 3) == 0 else 0.0
                if rng.integers(0, 4) == 0:
                    kx = -kx
                ox, oy = x0 + float(rng.uniform(-12, 56)), y0 + float(rng.uniform(-5, 6))       # the bitmap's corner in or just off the strip
            st = bitmap_style(0, extend, kx, ky, ox, oy, t)
            seen = strip_halves(st, rect, bw, bh, x0, y0)
            if inside and all(seen[h] == (True, True) for h in halves):
                break
            if cls == "bitmap_minified" and not seen[0][0]:
                break
            if cls.startswith("bitmap_rim") and seen[0][0] and not any(seen[h][1] for h in halves):
                break
        else:
            raise AssertionError("no matrix found for " + cls)
        st.bitmap = fr.add_bitmap(rand_texels(rng, bw, bh, opaque=cls == "bitmap_inside_plain"))
        return st

    def radial(rect):
        radius = float(rng.uniform(30, 48))
        stops = sorted((int(rng.integers(0, 256)), tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.choice([255, 255, 128, 0, 37])),)) for _ in range(int(rng.integers(1, 5))))
        focal = float(rng.uniform(-0.7, 0.7)) if rng.integers(0, 2) else 0.0
        return radial_style(int(rng.choice([1, 2, 1, 2, 0])), radius, x0 + 32 + float(rng.uniform(-14, 14)), y0 + 4 + float(rng.uniform(-5, 5)), stops, focal,
                            float(rng.uniform(-3.2, 3.2)) if rng.integers(0, 2) else 0.0)

    style = radial if cls == "radial_spread" else bitmap
    if geometry[0] == "rect":
        fr.rect_tor(*geometry[1], 0, lerp, op, style=style)
    elif geometry[0] == "box":
        fr.box(*geometry[1], 0, lerp, op, style=style)
    else:
        fr.tor(geometry[1], 0, lerp, op, style=style)


SHADED_MODES = ("plain", "lerp") + tuple(MODES[1:])      # unblended, the lerp bit as a first paint, each of the eight operators
SHADED_SETTINGS = ("alone", "group", "mask_content", "mask", "fade_1", "fade_128", "fade_254", "nested")
SHADED_BEHIND = (0, 15, 16, 17)                           # plain entries before it: either side of a staging round
SHADED_SIZES = (((130, 21), ((0, 0), (64, 8), (0, 8), (128, 16), (64, 0))), ((70, 13), ((0, 0), (64, 8), (0, 8))))       # frame, strips


def shaded_frame(cls, mode, setting, k, size, strip, seed):
    """One frame: `k` plain solid entries in the strip, then one member of class `cls` -- unblended, with the lerp bit (a first paint:
    then nothing comes before it on its surface) or under the operator `mode` -- alone, in a group, as the content or as the mask of
    a masked group, in a faded group or two groups deep; a solid path on top."""
    rng = np.random.default_rng(seed)
    W, H = size
    x0, y0 = strip
    fr = RawFrame(W, H)
    lerp = mode == "lerp"
    op = "normal" if mode in ("plain", "lerp") else mode
    if lerp and setting == "alone":
        k = 0
    for i in range(k):
        add_member(fr, rng, ("full_translucent", "box", "partial")[i % 3], MODES[(seed + 2 * i) % 9] if i else "normal", x0, y0, first=i == 0)
    member = lambda: add_shaded_member(fr, rng, cls, op, x0, y0, lerp)
    end_op = MODES[seed % 9]
    if setting == "alone":
        member()
    elif setting == "group":
        fr.begin()
        member()
        add_member(fr, rng, "partial", MODES[(seed + 1) % 9], x0, y0)
        fr.end(end_op)
    elif setting == "mask_content":
        fr.begin()
        member()
        add_member(fr, rng, "box", MODES[(seed + 1) % 9], x0, y0)
        fr.mask()
        add_member(fr, rng, "partial", "normal", x0, y0, first=True)
        add_member(fr, rng, "full_translucent", "normal", x0, y0)
        fr.end(end_op)
    elif setting == "mask":
        fr.begin()
        add_member(fr, rng, "full_translucent", "normal", x0, y0, first=True)
        add_member(fr, rng, "partial", MODES[(seed + 1) % 9], x0, y0)
        fr.mask()
        member()
        fr.end(end_op)
    elif setting.startswith("fade"):
        fr.begin()
        member()
        add_member(fr, rng, "partial", MODES[(seed + 1) % 9], x0, y0)
        fr.end(end_op, opacity=int(setting.split("_")[1]))
    else:
        fr.begin()
        add_member(fr, rng, "partial", "normal", x0, y0, first=True)
        fr.begin()
        member()
        fr.end(MODES[(seed + 4) % 9])
        add_member(fr, rng, "box", MODES[(seed + 1) % 9], x0, y0)
        fr.end(end_op)
    add_member(fr, rng, "partial", MODES[(seed + 3) % 9], x0, y0)
    return fr


def shaded_frames(cls):
    """(label, frame) of one member class: every mode x every setting; the count of entries before it, the frame size and the strip
    go round"""
    ci = SHADED_CLASSES.index(cls)
    n = 0
    for mi, mode in enumerate(SHADED_MODES):
        for si, setting in enumerate(SHADED_SETTINGS):
            k = SHADED_BEHIND[(mi + si + ci) % 4]
            size, strips = SHADED_SIZES[(mi + si // 2) % 2]
            strip = strips[n % len(strips)]
            yield (cls, mode, setting, k, size, strip), shaded_frame(cls, mode, setting, k, size, strip, 7000 + 100 * ci + n)
            n += 1


def shaded_reach(frames):
    """What the wavefronts of the tile pass see of the shaded paths of `frames` (RawFrames), from the arrays, the coverage of
    tests/frame_model.py and the sample positions of tests/pad_model.py -- never from the kernel.  A dict of counts:
    per (path, strip, row half with coverage) of an unblended bitmap path  ("inside", plain) / ("general", extend) / ("convolution", extend)
        -- inside: all 256 samples strictly inside the bitmap; plain: coverage 255 at all of them and every source pixel opaque;
    per shaded path  ("lerp",), ("operator", name), ("setting", "group" | "mask_content" | "mask" | "faded" | "nested")"""
    import frame_model as fm
    import pad_model as pm
    out = {}

    def count(*key):
        out[key] = out.get(key, 0) + 1
    for fr in frames:
        edges, paths, styles = fr.arrays()
        texels = fr.model_bitmaps()
        ends, opened = {}, []                                        # BEGIN index -> (MASK index or None, END index)
        for i, p in enumerate(paths):
            kind = int(p["kind"])
            if kind == BEGIN:
                opened.append([i, None])
            elif kind == MASK:
                opened[-1][1] = i
            elif kind == END:
                b, m = opened.pop()
                ends[b] = (m, i)
        stack = []
        for i, p in enumerate(paths):
            kind = int(p["kind"])
            if kind == BEGIN:
                stack.append(i)
                continue
            if kind == END:
                stack.pop()
                continue
            st = styles[int(p["style"])]
            if kind == MASK or int(st.kind) == fm.STYLE_SOLID:
                continue
            field = int(p["lerp"])
            if field & 1:
                count("lerp")
            if field >> 8:
                count("operator", MODES[0] if not field >> 8 else fm.OPERATOR_NAMES[field >> 8])
            if stack:
                m, e = ends[stack[-1]]
                count("setting", "group" if m is None else ("mask_content" if i < m else "mask"))
                if int(paths[e]["lerp"]) >> 24:
                    count("setting", "faded")
                if len(stack) > 1:
                    count("setting", "nested")
            if int(st.kind) != fm.STYLE_BITMAP or field >> 8:
                continue
            rect, cov = fm.path_coverage(edges, p, fr.W, fr.H)
            bmp = texels[int(st.bitmap)]
            inv = tuple(float(v) for v in st.inv)
            for sy in range(rect[1] // STRIP_H * STRIP_H, rect[3], STRIP_H):
                for sx in range(rect[0] // STRIP_W * STRIP_W, rect[2], STRIP_W):
                    seen = strip_halves(st, tuple(int(p[k]) for k in ("x_min", "y_min", "x_max", "y_max")), bmp.shape[1], bmp.shape[0], sx, sy)
                    for h, (bilinear, inside) in enumerate(seen):
                        block = np.zeros((4, STRIP_W), np.uint8)                             # the half's coverage, zero outside the rectangle
                        ya, yb, xa, xb = max(sy + 4 * h, rect[1]), min(sy + 4 * h + 4, rect[3]), max(sx, rect[0]), min(sx + STRIP_W, rect[2])
                        if ya < yb and xa < xb:
                            block[ya - sy - 4 * h:yb - sy - 4 * h, xa - sx:xb - sx] = cov[ya - rect[1]:yb - rect[1], xa - rect[0]:xb - rect[0]]
                        if not block.any():
                            continue                                 # (the kernel skips a half without coverage as a whole)
                        if not bilinear:
                            count("convolution", int(st.extend))
                        elif not inside:
                            count("general", int(st.extend))
                        else:
                            src = pm.source_pixels(inv, bmp, (sx, sy + 4 * h, sx + STRIP_W, sy + 4 * h + 4), int(st.extend),
                                                   tuple(int(p[k]) for k in ("x_min", "y_min", "x_max", "y_max")))
                            count("inside", bool((block == 255).all() and ((src >> 24) == 255).all()))
    return out


def assert_shaded_reach(rc, least=5):
    """every branch of the bitmap fetch and every place a shaded member can stand, each at least `least` times"""
    need = [("inside", True), ("inside", False), ("lerp",)] + [(f, e) for f in ("general", "convolution") for e in (0, 1, 2)]
    need += [("operator", m) for m in MODES[1:]] + [("setting", s) for s in ("group", "mask_content", "mask", "faded", "nested")]
    for key in need:
        assert rc.get(key, 0) >= least, (key, rc.get(key, 0))


def lerp_beside_painted_frame(seed, W=130, H=21):
    """A bitmap path with the lerp bit whose own rectangle is still clear while the rest of its strip is not: solid boxes right of
    column 38 and below row 8, then the bitmap -- a box off the pixel grid or a triangle -- left of them.  A lerp ignores its
    destination, so the pixels of the strip outside the path have to be kept lane by lane."""
    rng = np.random.default_rng(7950 + seed)
    fr = RawFrame(W, H)
    fr.box(38, 0, 64 + float(rng.uniform(3, 40)), 7.5, premultiplied(rng, int(rng.integers(60, 255))), 1)
    fr.rect_tor(0, 9, W, 14, premultiplied(rng, int(rng.integers(60, 255))), 0, MODES[seed % 9])
    bw, bh = ((7, 7), (3, 3), (47, 48), (2, 2))[seed % 4]
    bid = fr.add_bitmap(rand_texels(rng, bw, bh, opaque=seed % 3 == 0))
    k = 70.0 / max(bw - 1, 1) if seed % 2 else float(rng.uniform(0.9, 6))
    style = lambda rect: bitmap_style(bid, seed % 3, k, k, -1.5 - (k if seed % 2 else 0) * 0.6, -2.25 - (k if seed % 2 else 0) * 0.2)
    if seed % 2:
        fr.box(1.3, 0.6, 36.4, 7.7, 0, 1, style=style)
    else:
        fr.tor([(2.2, 0.4), (37.1, 3.3), (9.6, 7.8)], 0, 1, style=style)
    add_member(fr, rng, "partial", MODES[(seed + 3) % 9], 0, 0)
    return fr


def last_column_frame(seed, W=70, H=13):
    """Whole rows of the first strip filled from a bitmap so placed that the samples' left taps run up to the bitmap's LAST column and
    no further (their right taps are then outside it: wrapped, clamped or transparent), every row tap inside: one column short of the
    all-inside shortcut.  -> (frame, the set of left-tap columns of the strip's samples, the bitmap's width)"""
    import spread_model as sm
    rng = np.random.default_rng(7970 + seed)
    fr = RawFrame(W, H)
    if seed % 2:
        fr.rect_tor(-1, -1, W + 1, H + 1, premultiplied(rng, int(rng.integers(40, 255))), 1)
    bw, bh = ((2, 4), (3, 5), (7, 7), (5, 4))[seed % 4]
    bid = fr.add_bitmap(rand_texels(rng, bw, bh, opaque=seed % 5 == 0))
    kx, ky = float(rng.uniform(72, 88)), 12.0
    st = bitmap_style(bid, seed % 3, kx, ky, 0.5 - kx * (bw - 1.1), 0.5 - ky * 1.0)
    fr.rect_tor(0, 0, STRIP_W + 2, 8, 0, 0 if seed % 2 else 1, style=lambda rect: st)
    (bx, by), ((m00, m01), (m10, m11)) = sm.to_pixman(tuple(st.inv), fr.paths[-1][6:10])
    px, py = np.meshgrid(np.arange(STRIP_W, dtype=np.int64), np.arange(8, dtype=np.int64))
    ty = (by + px * m10 + py * m11 - 0x8000) >> 16
    assert ty.min() >= 0 and ty.max() <= bh - 3
    return fr, set(((bx + px * m00 + py * m01 - 0x8000) >> 16).ravel().tolist()), bw
