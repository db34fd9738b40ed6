"""tests/fade_model.py -- the layer-opacity rule in numpy -- against live libcairo, pixel by pixel: a real cairo_push_group /
cairo_pop_group_to_source / cairo_set_operator / cairo_paint_with_alpha on an n x 1 surface, for each of the nine operators, four kinds
of parent and ALL 256 opacities; and libcairo's clear-surface bookkeeping behind the call.  No GPU.  Skipped where libcairo is absent."""
import ctypes

import numpy as np
import pytest

import blend_model as bm
from cairo_pixels import random_premultiplied, surface_bytes
import fade_model as fd
import layer_model as lm
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
N = 1024                                   # pixels (= random pairs) per operator, destination kind and opacity
CAIRO_OPERATOR_OVER = 2


def _declare(lib):
    P, D = ctypes.c_void_p, ctypes.c_double
    for fn, res, args in (("cairo_push_group", None, [P]), ("cairo_pop_group_to_source", None, [P]), ("cairo_get_group_target", P, [P]),
                          ("cairo_paint_with_alpha", None, [P, D])):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args


def _fade(dst, group, operator, opacity, n, probe=None):
    """an n x 1 surface holding `dst` (None: a cleared surface nothing was drawn on); a group holding `group` (written into its surface:
    the surface counts as drawn on; None: a still-clear group) painted onto it under `operator` with cairo_paint_with_alpha.  `probe`:
    a translucent wedge then filled across the surface with OVER -- on a surface libcairo still takes for clear that is a SOURCE lerp,
    otherwise OVER (tests/test_mask_model.py's technique)."""
    be = cb.CairoBackend(n, 1)
    lib, cr = be.lib, be.cr
    _declare(lib)
    try:
        be.clear_all()
        if dst is not None:
            surface_bytes(be)[0] = dst[:, [2, 1, 0, 3]]
            lib.cairo_surface_mark_dirty(be.surf)
        lib.cairo_push_group(cr)
        if group is not None:
            target = lib.cairo_get_group_target(cr)
            lib.cairo_surface_flush(target)
            stride = lib.cairo_image_surface_get_stride(target)
            data = np.ctypeslib.as_array(lib.cairo_image_surface_get_data(target), shape=(1, stride))
            data[0, : n * 4] = group[:, [2, 1, 0, 3]].reshape(-1)
            lib.cairo_surface_mark_dirty(target)
        lib.cairo_pop_group_to_source(cr)
        lib.cairo_set_operator(cr, operator)
        lib.cairo_paint_with_alpha(cr, opacity / 255.0)
        assert lib.cairo_status(cr) == 0
        out = be.premultiplied_rgba()[0].copy()
        if probe is not None:
            lib.cairo_set_operator(cr, CAIRO_OPERATOR_OVER)
            lib.cairo_set_source_rgba(cr, *[v / 255.0 for v in probe])
            lib.cairo_move_to(cr, 0, 0)                      # (a wedge: the coverage runs from 0 to 255 along the row)
            lib.cairo_line_to(cr, n, 0)
            lib.cairo_line_to(cr, n, 1)
            lib.cairo_fill(cr)
            return out, be.premultiplied_rgba()[0].copy()
        return out
    finally:
        be.close()


def _group(rng, n):
    group = random_premultiplied(rng, n, "translucent")
    group[n // 2: n // 2 + n // 16] = random_premultiplied(rng, n // 16, "opaque")
    group[-n // 16:] = 0
    return group


@needs_cairo
@pytest.mark.parametrize("mode", sorted(fd.MODES))
@pytest.mark.parametrize("ground", ["opaque", "translucent", "clear_pixels", "still_clear"])
def test_model_is_libcairo_at_every_opacity(mode, ground):
    rng = np.random.default_rng(sorted(fd.MODES).index(mode) * 11 + 41)
    group = np.stack([_group(rng, N) for _ in range(4)])                     # (the rows of pairs take turns over the opacities)
    # ("clear_pixels": transparent pixels of a surface that has been drawn on; "still_clear": Cairo's still-clear surface)
    dst = None if ground == "still_clear" else np.stack([random_premultiplied(rng, N, "clear" if ground == "clear_pixels" else ground) for _ in range(4)])
    d = np.zeros((4, N, 4), np.uint8) if dst is None else dst
    rows = np.arange(256) % 4
    got = np.stack([_fade(None if dst is None else dst[k % 4], group[k % 4], bm.CAIRO_OPERATORS[mode], k, N) for k in range(256)])
    want = fd.composite(mode, group[rows], np.arange(256).reshape(256, 1, 1), d[rows])
    bad = np.argwhere((got != want).any(-1))
    assert len(bad) == 0, "%d of %d pixels differ, first: opacity %d group %s dst %s cairo %s model %s" % (
        len(bad), 256 * N, bad[0][0], group[bad[0][0] % 4, bad[0][1]], d[bad[0][0] % 4, bad[0][1]], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (got != d[rows]).any(-1).sum() > 128 * N          # (the operator did something)
    assert (got[:, -N // 16:] == d[rows][:, -N // 16:]).all()   # a transparent group pixel leaves the destination as it is
    assert (got[0] == d[0]).all()                            # opacity 0 leaves the parent as it is


def test_opacity_255_is_the_plain_layer_and_0_is_nothing():
    rng = np.random.default_rng(9)
    group = _group(rng, 20000)
    for kind in ("translucent", "opaque", "clear"):
        d = random_premultiplied(rng, 20000, kind)
        for mode in fd.MODES:
            assert (fd.composite(mode, group, 255, d) == lm.composite(mode, group, d)).all(), (mode, kind)
            assert (fd.composite(mode, group, 0, d) == d).all(), (mode, kind)
            for opacity in (1, 128, 254):
                assert (fd.composite(mode, np.zeros_like(group), opacity, d) == d).all(), (mode, kind, opacity)
    # every channel fades, alpha included, with 0x80 rounding -- not 0x7f, not truncation: 1 * 128 / 255 rounds to 1, 1 * 127 / 255 to 0
    assert fd.faded(np.array([[1, 1, 1, 1]], np.uint8), 128).tolist() == [[1, 1, 1, 1]]
    assert fd.faded(np.array([[1, 1, 1, 1]], np.uint8), 127).tolist() == [[0, 0, 0, 0]]
    assert fd.faded(np.array([[200, 100, 50, 255]], np.uint8), 128).tolist() == [[100, 50, 25, 128]]
    assert fd.end_lerp(7, 255) == 7 << 8 and fd.end_lerp(0, 0) == 0xff000000 and fd.end_lerp(3, 128) == (127 << 24) | (3 << 8)


@needs_cairo
@pytest.mark.parametrize("mode", sorted(fd.MODES))
def test_clear_surface_bookkeeping_is_libcairos(mode):
    """On a still-clear parent: the pixels after cairo_paint_with_alpha, and whether libcairo still takes the parent for clear -- seen
    in a translucent fill behind it, a SOURCE lerp on a clear surface (the premultiplied colour itself) and OVER otherwise.  The group
    still clear, or drawn on with every pixel zero; opacities 0, 1, 128, 254 and 255."""
    n = 512
    zero = np.zeros((n, 4), np.uint8)
    probe = (97, 184, 252, 38)             # (0x7f and 0x80 rounding differ at one coverage value per channel value at most: this colour has one)
    lerp = _fade(None, None, CAIRO_OPERATOR_OVER, 255, n, probe)[1]           # nothing at all happened to the parent
    over = _fade(random_premultiplied(np.random.default_rng(1), n, "clear"), None, CAIRO_OPERATOR_OVER, 255, n, probe)[1]   # a drawn-on parent
    assert (lerp != over).any()                              # (the probe tells the two states apart)
    for group_clear in (True, False):
        for opacity in (0, 1, 128, 254, 255):
            out, after = _fade(None, None if group_clear else zero, bm.CAIRO_OPERATORS[mode], opacity, n, probe)
            assert (out == 0).all()
            stays = fd.parent_stays_clear(mode, group_clear, opacity)
            assert (after == (lerp if stays else over)).all(), (mode, group_clear, opacity, stays)
            if opacity == 255:
                assert stays == lm.parent_stays_clear(mode, group_clear)
    # a parent that was drawn on stays drawn on, at opacity 0, too
    d = random_premultiplied(np.random.default_rng(2), n, "clear")
    for opacity in (0, 128):
        assert (_fade(d, None, bm.CAIRO_OPERATORS[mode], opacity, n, probe)[1] == over).all()
