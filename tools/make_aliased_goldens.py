"""Generates tests/golden/cairo_aliased_*.npz: what libcairo 1.16 renders under CAIRO_ANTIALIAS_NONE (node-canvas's
ctx.antialias = 'none'), the reference of SWFR_FLAG_ANTIALIAS_NONE / Renderer(antialias="none").  Needs the system libcairo; the
outputs are data and are committed, so the tests on the GPU box need no libcairo.  The scenes are rebuilt by the tests from the
functions below (tests/test_aliased.py imports this module), so a golden file holds pixels only.

  cairo_aliased_<scenario>.npz   every tests/scenarios.py scenario (key rgba_premul)
  cairo_aliased_probes.npz       the rule's edge cases: half-pixel edges, one- and two-pixel gaps, rounded boxes (key = probe name)
  cairo_aliased_random.npz       seeded random scenes of tests/helpers.rand_mixed_scene (key mixed_<seed>)
  cairo_aliased_combs.npz        rows with 2 200 and 6 000 active edges of one path, both fill rules (key comb_<teeth>_<rule>)
  cairo_aliased_wide.npz         a frame wider than 8 192 px, a few rows tall (key wide_<k>)
  cairo_aliased_s1.npz           S1 at 4K: sha256 of the premultiplied frame (key sha256) and five 256 x 256 crops (key x_y)
  cairo_aliased_extreme.npz      tests/helpers.extreme_scene frames, geometry at the +-2^23 limits, three per LARGE_MODES entry (key <mode>_<k>)

usage: python tools/make_aliased_goldens.py [--check] [--only NAME ...]    (--check: regenerate in memory and compare with the committed
       files; --only: just the named files, e.g. --only cairo_aliased_extreme)
"""
import hashlib
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import cairo_backend as cb, canvas_replay as cr  # noqa: E402
from swf_renderer_amd import synth  # noqa: E402
import scenarios  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CAIRO_ANTIALIAS_NONE = 1
RANDOM_SEEDS = range(40)
COMB_TEETH = (1100, 3000)            # 2 200 and 6 000 active edges in every row
S1_CROPS = ((0, 0), (2432, 768), (1792, 1024), (3584, 1904), (960, 320))
U = 256                              # probes are drawn in twips under scale(20 / 256): one unit = 1/256 px, Cairo's own grid


def aliased_backend(width, height):
    """A CairoBackend whose context draws with CAIRO_ANTIALIAS_NONE (set before the replay; save/restore keep it)."""
    import ctypes
    be = cb.CairoBackend(width, height)
    f = be.lib.cairo_set_antialias
    f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
    f(be.cr, CAIRO_ANTIALIAS_NONE)
    return be


def cairo_aliased(sc):
    """premultiplied RGBA of a scenario dict (tests/scenarios.py format) through libcairo under CAIRO_ANTIALIAS_NONE"""
    be = aliased_backend(sc["width"], sc["height"])
    if sc.get("even_odd"):
        be.set_fill_rule(True)
    rp = cr.CanvasReplay(be, linear_extension=True)
    for b in sc.get("bitmaps", []):
        rp.add_bitmap(b)
    rp.render(sc["stage"])
    out = be.premultiplied_rgba()
    be.close()
    return out


def multi_poly_shape(polys, fill):
    """DefineShape with several closed polygons (integer twips) in ONE fill style: one path of several sub-paths"""
    recs = []
    for poly in polys:
        p = [(int(x), int(y)) for x, y in poly]
        sc = {"type": "style-change", "move_to": {"x": p[0][0], "y": p[0][1]}}
        if not recs:
            sc["left_fill"] = 1
        recs.append(sc)
        for k in range(1, len(p) + 1):
            a, b = p[k - 1], p[k % len(p)]
            recs.append({"type": "edge", "delta": {"x": b[0] - a[0], "y": b[1] - a[1]}})
    xs = [int(q[0]) for poly in polys for q in poly]
    ys = [int(q[1]) for poly in polys for q in poly]
    return {"id": 1, "bounds": {"x_min": min(xs), "x_max": max(xs), "y_min": min(ys), "y_max": max(ys)},
            "shape": {"initial_styles": {"fill": [fill], "line": []}, "records": recs}}


def _fine(w, h, polys, color=(30, 60, 200, 255), even_odd=False):
    """a probe: polygons in 1/256 px under scale(20/256), one path"""
    s = 20.0 / U
    tag = multi_poly_shape(polys, {"type": "solid", "color": scenarios._rgba(*color)})
    return dict(width=w, height=h, even_odd=even_odd, stage={"children": [{"type": "shape", "definition": tag, "matrix": scenarios._m(s, s)}]})


def probe_scenarios():
    out = {}
    for f in (127, 128, 129):
        x = 5 * U + f
        # a vertical LEFT edge at 5 + f/256 (pixel 5 covered for f <= 128), the right side slanted
        out["vleft_%d" % f] = _fine(24, 8, [[(x, U), (15 * U, U), (18 * U, 7 * U), (x, 7 * U)]])
        # a vertical RIGHT edge (pixel 5 covered for f >= 129)
        out["vright_%d" % f] = _fine(24, 8, [[(1 * U, U), (x, U), (x, 7 * U), (3 * U, 7 * U)]])
        # a horizontal TOP edge at y = f/256 (row 0 covered for f <= 128)
        out["top_%d" % f] = _fine(24, 8, [[(2 * U, f), (12 * U, f), (16 * U, 6 * U), (1 * U, 6 * U)]])
        # a slanted edge through a row centre at a pixel boundary + f/256
        out["slant_%d" % f] = _fine(24, 8, [[(2 * U, 0), (6 * U + f - U // 2, 0), (6 * U + f + U // 2, 2 * U), (2 * U, 2 * U)]])
        # rectilinear paths (boxes, rounded to whole pixels): an L shape, two overlapping rectangles, with coordinates at k + f/256
        out["box_L_%d" % f] = _fine(24, 12, [[(2 * U + f, 1 * U + f), (9 * U + f, 1 * U + f), (9 * U + f, 4 * U + f), (5 * U + f, 4 * U + f),
                                             (5 * U + f, 10 * U + f), (2 * U + f, 10 * U + f)]])
        out["box_overlap_%d" % f] = _fine(24, 12, [[(2 * U + f, 1 * U + f), (9 * U + f, 1 * U + f), (9 * U + f, 6 * U + f), (2 * U + f, 6 * U + f)],
                                                   [(6 * U + f, 3 * U + f), (14 * U + f, 3 * U + f), (14 * U + f, 9 * U + f), (6 * U + f, 9 * U + f)]])
        out["box_overlap_evenodd_%d" % f] = dict(out["box_overlap_%d" % f], even_odd=True)
    # one path, two slanted pieces that leave pixel 10 uncovered at its centre: the span goes on (one-pixel gap filled) ...
    a = [(2 * U, U), (10 * U + 77, U), (10 * U + 100, 6 * U), (2 * U, 6 * U)]
    out["gap_one"] = _fine(24, 8, [a, [(11 * U + 100, U), (20 * U, U), (20 * U, 6 * U), (11 * U + 77, 6 * U)]])
    # ... a two-pixel gap stays open
    out["gap_two"] = _fine(24, 8, [a, [(12 * U + 100, U), (20 * U, U), (20 * U, 6 * U), (12 * U + 77, 6 * U)]])
    # two rectangles of one rectilinear path a pixel apart: boxes keep the gap
    out["gap_boxes"] = _fine(24, 8, [[(2 * U, U), (10 * U, U), (10 * U, 6 * U), (2 * U, 6 * U)], [(11 * U, U), (20 * U, U), (20 * U, 6 * U), (11 * U, 6 * U)]])
    # a box that rounds away, then a translucent fill (the "still clear" state of the surface)
    thin = _fine(24, 8, [[(3 * U + 130, U), (3 * U + 200, U), (3 * U + 200, 6 * U), (3 * U + 130, 6 * U)]])
    over = _fine(24, 8, [[(1 * U, 2 * U), (14 * U, 2 * U + 90), (12 * U, 7 * U)]], color=(200, 100, 50, 120))
    out["box_rounds_away_then_translucent"] = dict(thin, stage={"children": thin["stage"]["children"] + over["stage"]["children"]})
    # gaps and pieces in both fill rules: a star with a hole
    star = [(int(12 * U + 9 * U * np.cos(2.513274 * k)), int(8 * U + 7 * U * np.sin(2.513274 * k))) for k in range(5)]
    out["star_evenodd"] = _fine(24, 16, [star], even_odd=True)
    out["star_nonzero"] = _fine(24, 16, [star])
    return out


def random_scene(seed):
    from helpers import rand_mixed_scene
    return rand_mixed_scene(np.random.default_rng(1000 + seed))


def comb_points(teeth, width_twips):
    pts = []
    step = width_twips / teeth
    for k in range(teeth):
        pts += [(100 + step * k, 100), (100 + step * k + step / 2, 1900)]
    pts += [(100 + width_twips + 100, 1950), (50, 1950)]
    return pts


def comb_scene(teeth, even_odd, width_twips=6000):
    tag = scenarios._poly_shape(comb_points(teeth, width_twips), {"type": "solid", "color": scenarios._rgba(1, 2, 3)})
    return dict(width=320, height=100, even_odd=even_odd, stage={"children": [{"type": "shape", "definition": tag}]})


def wide_scenes():
    """frames 9 600 px wide, 24 rows: paths wider than the 8 192 columns of a cell, and one beyond them"""
    w, h = 9600, 24
    far = scenarios._poly_shape([(9000 * 20 + 7, 50), (9500 * 20 + 3, 150), (9200 * 20, 450)], {"type": "solid", "color": scenarios._rgba(200, 100, 50, 160)})
    pts = [(100, 50), (9400 * 20, 100), (9400 * 20, 350), (100, 300), (3000 * 20, 175)]
    wide = scenarios._poly_shape(pts, {"type": "solid", "color": scenarios._rgba(200, 30, 90, 140)})
    sliver = scenarios._poly_shape([(100, 200), (9590 * 20, 235), (9590 * 20, 260), (100, 215)], {"type": "solid", "color": scenarios._rgba(10, 90, 250, 200)})
    return {"wide_%d" % k: dict(width=w, height=h, stage={"children": [{"type": "shape", "definition": d} for d in kids]})
            for k, kids in enumerate(([wide], [wide, sliver, far]))}


def extreme_scenes():
    """three seeded extreme_scene frames of each LARGE_MODES entry, 64 x 48 and 333 x 97 in turn"""
    from helpers import LARGE_MODES, extreme_scene
    out = {}
    for mode in LARGE_MODES:
        rng = np.random.default_rng(zlib.crc32(("aliased golden " + mode).encode()) % 1000)
        for k in range(3):
            out["%s_%d" % (mode, k)] = extreme_scene(rng, *[(64, 48), (333, 97)][k % 2], mode)
    return out


def s1_image():
    pts, cols = synth.scene(**synth.S1)
    from swf_renderer_amd import api
    return cairo_aliased(dict(width=synth.S1["width"], height=synth.S1["height"], stage=api.stars_to_stage(pts, cols)))


def generate(only=None):
    """name -> {key: array} of every golden file (of the named ones only)"""
    if only:
        return {name: _extreme() if name == "cairo_aliased_extreme" else generate()[name] for name in only}
    files = {}
    for name, sc in scenarios.scenarios().items():
        files["cairo_aliased_" + name] = {"rgba_premul": cairo_aliased(sc)}
    files["cairo_aliased_probes"] = {k: cairo_aliased(sc) for k, sc in probe_scenarios().items()}
    files["cairo_aliased_random"] = {"mixed_%d" % s: cairo_aliased(random_scene(s)) for s in RANDOM_SEEDS}
    files["cairo_aliased_combs"] = {"comb_%d_%s" % (t, "evenodd" if eo else "nonzero"): cairo_aliased(comb_scene(t, eo))
                                    for t in COMB_TEETH for eo in (False, True)}
    files["cairo_aliased_wide"] = {k: cairo_aliased(sc) for k, sc in wide_scenes().items()}
    img = s1_image()
    s1 = {"sha256": np.array(hashlib.sha256(img.tobytes()).hexdigest())}
    for (x, y) in S1_CROPS:
        s1["%d_%d" % (x, y)] = img[y:y + 256, x:x + 256].copy()
    files["cairo_aliased_s1"] = s1
    files["cairo_aliased_extreme"] = _extreme()
    return files


def _extreme():
    return {k: cairo_aliased(sc) for k, sc in extreme_scenes().items()}


def main():
    assert cb.available(), "libcairo is required to generate goldens"
    check = "--check" in sys.argv
    only = sys.argv[sys.argv.index("--only") + 1:] if "--only" in sys.argv else None
    bad = []
    for name, arrays in generate(only).items():
        path = os.path.join(OUT, name + ".npz")
        if check:
            old = np.load(path)
            if sorted(old.files) != sorted(arrays) or any(not np.array_equal(old[k], v) for k, v in arrays.items()):
                bad.append(name)
        else:
            np.savez_compressed(path, **arrays)
            print(name, ", ".join("%s %s" % (k, v.shape) for k, v in list(arrays.items())[:3]))
    if check:
        print("differing:", bad or "none")
        sys.exit(1 if bad else 0)
    print("cairo", cb.version())


if __name__ == "__main__":
    main()
