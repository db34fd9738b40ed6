"""tests/spread_model.py -- pixman's radial gradient under REPEAT and REFLECT in Python integers and numpy.float32 -- against the
committed libcairo goldens of the exact-sample boxes and against live libcairo on random stops and matrices (skipped where libcairo is
absent), zero differing bytes; and the count DESIGN.md quotes: on how many pixels a walker that keeps its state along the scanline
(libcairo's, the rule) and a fresh reset per pixel disagree.  No GPU, no product code."""
import ctypes

import numpy as np
import pytest

import spread_model as sm
import spread_scenes as ss

EXTEND = {"reflect": sm.REFLECT, "repeat": sm.REPEAT}
CASES = 2000                                     # per gradient kind and spread, against live libcairo


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
