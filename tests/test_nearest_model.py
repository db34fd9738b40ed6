"""tests/nearest_model.py -- the source pixel of an unsmoothed bitmap fill (CAIRO_FILTER_NEAREST) and the rectangle an EXTEND_NONE one
is cut to -- against live libcairo (no GPU).

Pixels: random pixel-aligned boxes on a still-clear surface (tests/pad_scenes.py's random_box_case with the filter set), so that the
frame holds the source samples themselves: 2 400 padded, 300 each for none and repeat, zero differing bytes.  The same boxes go to the
device in tests/test_nearest_gpu.py, held against the model there.

The cut: libcairo shows it directly -- a large rectangle filled with the pattern on a cairo_recording_surface, read back with
cairo_recording_surface_ink_extents -- on the five measured rows of DESIGN.md's table (both filters) and on random matrices.  (A
recording surface is a vector target: where the rectangle rounds to nothing on an axis libcairo gives it one pixel there, and nothing
at all on an image surface.  The model has both rules; the boxes above hold the image surface's.)"""
import ctypes as C
import math

import numpy as np
import pytest

import nearest_model as nm
import nearest_scenes as ns
import spread_model as sm
from oracle import cairo_backend as cb

pytestmark = pytest.mark.skipif(not cb.available(), reason="needs the system libcairo")

CASES = 2400
PLACES = ("inside", "rim", "outside")


def _kind(places):
    return "inside" if places["outside"] == 0 else ("outside" if places["inside"] == 0 else "rim")


def _boxes(seed, n, extend, name):
    rng = np.random.default_rng(seed)
    seen = {(m, k): 0 for m in ("minified", "not") for k in PLACES}
    bad = 0
    for it in range(n):
        case = ns.random_box_case(rng, name, minified=bool(it & 1))
        md = case["model"]
        want, src = nm.frame(md["matrices"], nm.premultiply(md["bitmap"]), md["rect"], extend, ns.FW, ns.FH)
        assert src is not None
        seen["minified" if case["minified"] else "not", _kind(src["placements"]) if src["rect"] else "outside"] += 1
        got = ns.cairo_render(case["scene"])
        d = int((got != want).sum())
        if d:
            bad += 1
            print("case", it, name, case["aim"], md["matrices"], md["rect"], md["bitmap"].shape, "differing bytes", d)
    print(name, "classes", seen)
    assert bad == 0, "%d of %d %s boxes differ from libcairo" % (bad, n, name)
    return seen


def test_the_model_is_libcairo_on_random_padded_boxes():
    seen = _boxes(20261020, CASES, nm.PAD, "pad")
    assert all(n >= 200 for n in seen.values()), seen


@pytest.mark.parametrize("name", ["none", "repeat"])
def test_the_model_is_libcairo_under_the_other_two_rules(name):
    """EXTEND_NONE: the operation is cut to the bitmap's rectangle (nearest_model.cut_rect), which moves pixman's anchor with it"""
    _boxes(177 + len(name), 300, {"none": nm.NONE, "repeat": nm.REPEAT}[name], name)


# ---------------------------------------------------------------------------------------------------------------- the cut
def ink_extents(m, width, height, cairo_filter):
    """what libcairo bounds an EXTEND_NONE fill of a width x height bitmap by: (x0, y0, x1, y1); m: the pattern matrix"""
    lib = cb._load()
    P, D, I = C.c_void_p, C.c_double, C.c_int
    for fn, res, args in (("cairo_recording_surface_create", P, [I, P]), ("cairo_recording_surface_ink_extents", None, [P] + [C.POINTER(D)] * 4),
                          ("cairo_pattern_set_matrix", None, [P, P])):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args
    img = lib.cairo_image_surface_create(0, width, height)
    data, stride = lib.cairo_image_surface_get_data(img), lib.cairo_image_surface_get_stride(img)
    C.memset(data, 0xff, stride * height)
    lib.cairo_surface_mark_dirty(img)                             # (a clear source is a no-op: the bitmap must count as drawn on)
    rec = lib.cairo_recording_surface_create(0x3000, None)        # CAIRO_CONTENT_COLOR_ALPHA, unbounded
    cr = lib.cairo_create(rec)
    pat = lib.cairo_pattern_create_for_surface(img)
    mat = cb._Matrix(*m)
    lib.cairo_pattern_set_matrix(pat, C.byref(mat))
    lib.cairo_pattern_set_extend(pat, 0)
    lib.cairo_pattern_set_filter(pat, cairo_filter)
    lib.cairo_set_source(cr, pat)
    lib.cairo_rectangle(cr, -500.0, -500.0, 1000.0, 1000.0)
    lib.cairo_fill(cr)
    v = [D() for _ in range(4)]
    lib.cairo_recording_surface_ink_extents(rec, *[C.byref(x) for x in v])
    lib.cairo_destroy(cr)
    lib.cairo_pattern_destroy(pat)
    lib.cairo_surface_destroy(rec)
    lib.cairo_surface_destroy(img)
    x, y, w, h = [int(round(x.value)) for x in v]
    return x, y, x + w, y + h


TABLE = [  # k, off, GOOD, NEAREST: a 5 x 4 bitmap with device = k * texel + off
    (3, 10.3, (9, 9, 27, 24), (10, 10, 25, 22)),
    (3, 10.5, (9, 9, 27, 24), (10, 10, 26, 23)),
    (0.5, 10.3, (10, 10, 13, 13), (10, 10, 13, 12)),
    (1, 10.3, (10, 10, 16, 15), (10, 10, 15, 14)),
    (7.3, 4.9, (1, 1, 45, 38), (5, 5, 41, 34)),
]


@pytest.mark.parametrize("k,off,good,nearest", TABLE)
def test_the_cut_of_the_measured_table(k, off, good, nearest):
    m = sm.invert((float(k), 0.0, 0.0, float(k), off, off))
    assert nm.cut_rect(m, 5, 4, nearest=True) == nearest
    assert nm.cut_rect(m, 5, 4, nearest=False) == good
    assert ink_extents(m, 5, 4, nm.CAIRO_FILTER[nm.NEAREST]) == nearest
    assert ink_extents(m, 5, 4, nm.CAIRO_FILTER[nm.GOOD]) == good


def test_the_cut_on_random_matrices():
    rng = np.random.default_rng(436)
    n = 0
    for it in range(240):
        kx, ky = (float(np.exp(rng.uniform(math.log(0.3), math.log(12.0)))) for _ in range(2))
        t = float(rng.uniform(-3.2, 3.2)) if it % 3 else 0.0
        ox, oy = float(rng.uniform(-20, 60)), float(rng.uniform(-20, 60))
        w, h = int(rng.integers(1, 10)), int(rng.integers(1, 10))
        m = sm.invert((kx * math.cos(t), kx * math.sin(t), -ky * math.sin(t), ky * math.cos(t), ox, oy))
        assert m is not None
        # (the probe's target is a vector surface, where an axis that rounds to nothing is given one pixel: the model's is_vector)
        got = ink_extents(m, w, h, nm.CAIRO_FILTER[nm.NEAREST])
        assert nm.cut_rect(m, w, h, is_vector=True) == got, (it, kx, ky, t, ox, oy, w, h)
        cut = nm.cut_rect(m, w, h)
        if cut[0] < cut[2] and cut[1] < cut[3]:                   # nothing rounds away: the rectangle an image surface is cut to
            assert cut == got
            n += 1
    assert n >= 200
