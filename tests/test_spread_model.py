"""tests/spread_model.py -- pixman's radial gradient under REPEAT and REFLECT in Python integers and numpy.float32 -- against the
committed libcairo goldens of the exact-sample boxes and against live libcairo on random stops and matrices (skipped where libcairo is
absent), zero differing bytes; and the count DESIGN.md quotes: on how many pixels a walker that keeps its state along the scanline
(libcairo's, the rule) and a fresh reset per pixel disagree.  And the frame reference of the device fuzz (tests/spread_fuzz.py: spread_model.frame over a coverage
made without libcairo) against live libcairo's whole frame, on the generator's random cases and on the aimed run-start scenes, zero
differing bytes, with the count of caveat pixels -- where the device's every-sample rule paints otherwise.  No GPU, no kernel."""
import ctypes

import numpy as np
import pytest

import spread_model as sm
import spread_scenes as ss

EXTEND = {"reflect": sm.REFLECT, "repeat": sm.REPEAT}
CASES = 2000                                     # per gradient kind and spread, against live libcairo
FRAMES = 130                                     # per spread, kind, antialias mode and frame size: 1 560 frames a spread


@pytest.mark.parametrize("spread", ss.SPREADS)
def test_model_paints_the_exact_goldens(spread):
    total = {"samples on an interval end": 0, "on the left end of the walker's interval": 0, "pixels a fresh reset paints otherwise": 0}
    for aliased in (False, True):
        gold = np.load(ss.golden_path("cairo_spread_%s%s_exact" % ("aliased_" if aliased else "", spread)))
        for name, (sc, md) in sorted(ss.exact_cases(spread).items()):
            x0, y0, x1, y1 = md["rect"]
            out = sm.source(sm.pattern_matrix(md["matrices"]), md["circles"], md["stops"], EXTEND[spread], md["rect"])
            want = gold[name]
            assert (sm.rgba_bytes(out["stateful"]) == want[y0:y1, x0:x1]).all(), (name, aliased)
            inside = np.zeros(want.shape[:2], bool)
            inside[y0:y1, x0:x1] = True
            assert not want[~inside].any(), name
            if not aliased:
                for k, v in zip(total, (out["exact_hits"], out["on_left_end"], out["state_pixels"])):
                    total[k] += v
    print("spread model,", spread, "exact boxes:", total)
    assert total["samples on an interval end"] > 0
    if spread == "repeat":                       # only an odd period of REFLECT can tell the two walkers apart
        assert total["pixels a fresh reset paints otherwise"] == 0
    else:
        assert total["pixels a fresh reset paints otherwise"] > 0, "the exact boxes no longer tell a stateful walker from a fresh reset"


def _cairo_box(lib, matrix, circles, stops, extend, rect, w, h):
    """a pixel-aligned box filled with the radial gradient under cairo_scale(1/20) and the fill's matrix: premultiplied RGBA"""
    from oracle import cairo_backend as cb
    surf = lib.cairo_image_surface_create(0, w, h)
    cr = lib.cairo_create(surf)
    lib.cairo_rectangle(cr, rect[0], rect[1], rect[2] - rect[0], rect[3] - rect[1])
    lib.cairo_scale(cr, 1 / 20, 1 / 20)
    lib.cairo_transform(cr, ctypes.byref(cb._Matrix(*sm.swf_matrix(matrix))))
    pat = lib.cairo_pattern_create_radial(*circles)
    for o, r, g, b, a in stops:
        lib.cairo_pattern_add_color_stop_rgba(pat, o, r, g, b, a)
    lib.cairo_pattern_set_extend(pat, sm.CAIRO_EXTEND[extend])
    lib.cairo_set_source(cr, pat)
    lib.cairo_fill(cr)
    lib.cairo_surface_flush(surf)
    stride = lib.cairo_image_surface_get_stride(surf)
    buf = np.ctypeslib.as_array(lib.cairo_image_surface_get_data(surf), shape=(h, stride))[:, : w * 4].reshape(h, w, 4)
    out = np.ascontiguousarray(buf[..., [2, 1, 0, 3]])
    lib.cairo_pattern_destroy(pat)
    lib.cairo_destroy(cr)
    lib.cairo_surface_destroy(surf)
    return out


def _in_range(m, circles, rect):
    """the box maps within pixman's 16.16 range, relative to the centre and to the focus (tests/spread_scenes.py)"""
    for x in (rect[0], rect[2]):
        for y in (rect[1], rect[3]):
            u, v = sm.apply(m, float(x), float(y))
            if max(abs(u), abs(v), abs(u - circles[0]), abs(v - circles[1])) > 1.9 * ss.R:
                return False
    return True


@pytest.mark.parametrize("kind", ss.KINDS)
@pytest.mark.parametrize("spread", ss.SPREADS)
def test_model_is_libcairo_on_random_gradients(spread, kind):
    from oracle import cairo_backend as cb
    if not cb.available():
        pytest.skip("libcairo not available")
    lib = cb._load()
    rng = np.random.default_rng([ss.SPREADS.index(spread), ss.KINDS.index(kind), 2024])
    W, H, rect = 32, 8, (6, 2, 26, 5)
    done = state = ends = 0
    while done < CASES:
        radius = rng.uniform(7, 40)
        s = radius * 20 / ss.R
        matrix = ss._m(s, s * rng.uniform(0.6, 1.4), int(rng.integers(4 * 20, 28 * 20)), int(rng.integers(0, 8 * 20)), s * rng.uniform(-0.4, 0.4), s * rng.uniform(-0.4, 0.4))
        if rng.integers(0, 4) == 0:              # a centre on a pixel centre and a radius of whole pixels: samples on seams
            radius = int(rng.integers(6, 20))
            s = radius * 20 / ss.R
            matrix = ss._m(s, s, int(rng.integers(6, 26)) * 20 + 10, int(rng.integers(2, 5)) * 20 + 10)
        focal = {"radial": 0.0, "focal+": 1.0, "focal-": -1.0}[kind] * int(rng.integers(1, 250)) / 256.0
        circles = (focal * ss.R, 0.0, 0.0, 0.0, 0.0, ss.R)
        m = sm.pattern_matrix([matrix])
        if m is None or not _in_range(m, circles, rect):
            continue
        n = int(rng.integers(1, 7))
        ratios = sorted(int(v) for v in rng.choice([0, 0, 51, 102, 128, 204, 255, 255] + list(rng.integers(0, 256, 6)), n))
        stops = [(r / 255,) + tuple(int(c) / 255 for c in rng.integers(0, 256, 4)) for r in ratios]
        want = _cairo_box(lib, matrix, circles, stops, EXTEND[spread], rect, W, H)
        out = sm.source(m, circles, stops, EXTEND[spread], rect)
        x0, y0, x1, y1 = rect
        assert (sm.rgba_bytes(out["stateful"]) == want[y0:y1, x0:x1]).all(), (done, matrix, circles, stops)
        state += out["state_pixels"]
        ends += out["exact_hits"]
        done += 1
    print("spread model,", spread, kind, "random gradients:", CASES, "cases,", CASES * (rect[2] - rect[0]) * (rect[3] - rect[1]), "pixels,", ends,
          "samples on an interval end,", state, "pixels a fresh reset paints otherwise")


@pytest.mark.parametrize("kind", ss.KINDS)
@pytest.mark.parametrize("spread", ss.SPREADS)
def test_composed_frames_are_libcairo_on_random_cases(spread, kind):
    """what tests/test_spread_fuzz_gpu.py holds the device against (its cases are the first of these) is what libcairo paints: the whole
    frame, and the coverage that went into it"""
    from oracle import cairo_backend as cb
    if not cb.available():
        pytest.skip("libcairo not available")
    import spread_fuzz as sf
    done = caveat = covered = piecewise = 0
    shapes, strips, tiles, many_stops = {}, 0, 0, 0
    for aliased in (False, True):
        for size in sf.SIZES:
            for case in sf.cases(spread, kind, aliased, size, FRAMES):
                e = sf.expected(case)
                msg = (spread, kind, aliased, size, case["index"], case["shape"])
                assert (e["alpha"] == ss.cairo_render(case["white"], aliased)[..., 3]).all(), msg
                assert (e["truth"] == ss.cairo_render(case["scene"], aliased)).all(), msg
                assert not e["caveat"][e["alpha"] == 0].any()
                done += 1
                caveat += int(e["caveat"].sum())
                covered += int((e["alpha"] > 0).sum())
                piecewise += case["per_run"]
                shapes[case["shape"]] = shapes.get(case["shape"], 0) + 1
                sx, sy = sf.crossings(case)
                strips, tiles, many_stops = strips + sx, tiles + sy, many_stops + (len(case["model"]["stops"]) > 12)
    print("spread frames,", spread, kind, "random cases:", done, "frames,", covered, "covered pixels,", caveat, "caveat pixels;", shapes, piecewise,
          "composited piece by piece,", strips, "across a strip boundary,", tiles, "across a tile boundary,", many_stops, "with 13 to 16 stops")
    assert done == 4 * FRAMES and set(shapes) == set(sf.SHAPES) and strips and tiles and many_stops
    assert caveat <= covered // 1000, "caveat pixels are no longer rare: the device fuzz would be vacuous"


@pytest.mark.parametrize("spread", ss.SPREADS)
def test_composed_frames_are_libcairo_on_the_run_start_scenes(spread):
    """the aimed scenes: the composed frame is the committed golden (and live libcairo, where there is one); under REFLECT every scene
    has caveat pixels, those in the column its runs begin in at the rows the model named -- bar the `edge` scene, whose rectangle begins
    there: it shows libcairo's colour of the stepped scenes without a caveat, and the `mask` scene when antialiased, where one walker
    crosses the gap and arrives as the device's does; under REPEAT there is none"""
    from oracle import cairo_backend as cb
    import spread_fuzz as sf
    for aliased in (False, True):
        gold = np.load(ss.golden_path("cairo_spread_%s%s_runstart" % ("aliased_" if aliased else "", spread)))
        cases = ss.runstart_cases(spread, aliased)
        assert sorted(cases) == sorted(gold.files) and len(cases) >= 5 and {n.rsplit("_", 1)[1] for n in cases} >= {"gap", "mask", "edge"}
        for name, case in sorted(cases.items()):
            e = sf.expected(case)
            assert (e["truth"] == gold[name]).all(), (name, aliased)
            if cb.available():
                assert (gold[name] == ss.cairo_render(case["scene"], aliased)).all(), (name, aliased)
            where = [(int(y), int(x)) for y, x in np.argwhere(e["caveat"])]
            print("spread frames,", spread, "aliased" if aliased else "antialiased", name, "caveat pixels", where)
            assert where == ([(y, case["column"]) for y in case["rows"]] if spread == "reflect" and case["caveat"] else []), name
            if spread == "reflect" and case["edge"]:                 # libcairo's colour of the stepped scene, not the every-sample one
                step = sf.expected(cases[name[:-len("_edge")]])
                for y in case["rows"]:
                    at = (y, case["column"])
                    assert (gold[name][at] == step["truth"][at]).all() and (gold[name][at] != step["every_sample"][at]).any(), name
    # the runs begin in a strip other than the rectangle's first (64-pixel strips), and the scenes stay out of the exact routes
    assert any(c["model"]["rect"][0] // 64 != c["column"] // 64 for c in ss.runstart_cases(spread).values())
    assert not any(f.endswith("_runstart") for f in ss.files())
