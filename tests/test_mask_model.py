"""tests/mask_model.py -- the masked-layer rule in numpy -- against live libcairo, pixel by pixel: a real cairo_push_group /
cairo_pop_group twice, cairo_set_source, cairo_set_operator, cairo_mask on an n x 1 surface, for each of the nine operators and four
kinds of parent; and libcairo's clear-surface bookkeeping behind the call.  No GPU.  Skipped where libcairo is absent."""
import ctypes

import numpy as np
import pytest

import blend_model as bm
from cairo_pixels import random_premultiplied, surface_bytes
import mask_model as mk
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
N = 4096                                   # pixels (= random triples) per operator and ground kind
CAIRO_OPERATOR_OVER = 2


def _declare(lib):
    P = ctypes.c_void_p
    for fn, res, args in (("cairo_push_group", None, [P]), ("cairo_pop_group", P, [P]), ("cairo_get_group_target", P, [P]),
                          ("cairo_set_source", None, [P, P]), ("cairo_mask", None, [P, P]), ("cairo_pattern_destroy", None, [P]),
                          ("cairo_move_to", None, [P] + [ctypes.c_double] * 2), ("cairo_line_to", None, [P] + [ctypes.c_double] * 2), ("cairo_fill", None, [P]),
                          ("cairo_set_source_rgba", None, [P] + [ctypes.c_double] * 4)):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args


def _group(be, pixels, n):
    """a popped group holding `pixels` (written into its surface: the surface counts as drawn on), or -- None -- a still-clear one"""
    lib, cr = be.lib, be.cr
    lib.cairo_push_group(cr)
    if pixels is not None:
        target = lib.cairo_get_group_target(cr)
        lib.cairo_surface_flush(target)
        stride = lib.cairo_image_surface_get_stride(target)
        data = np.ctypeslib.as_array(lib.cairo_image_surface_get_data(target), shape=(1, stride))
        data[0, : n * 4] = pixels[:, [2, 1, 0, 3]].reshape(-1)
        lib.cairo_surface_mark_dirty(target)
    return lib.cairo_pop_group(cr)


def _mask(dst, content, mask, operator, n, probe=None):
    """an n x 1 surface holding `dst` (None: a cleared surface nothing was drawn on); a content group and a mask group (None: still
    clear) composited onto it with cairo_mask under `operator`.  `probe`: a translucent wedge then filled across the surface with
    OVER -- on a surface libcairo still takes for clear that is a SOURCE lerp (0x7f rounding in the premultiplication aside: the colour
    itself), otherwise OVER."""
    be = cb.CairoBackend(n, 1)
    lib, cr = be.lib, be.cr
    _declare(lib)
    try:
        be.clear_all()
        if dst is not None:
            surface_bytes(be)[0] = dst[:, [2, 1, 0, 3]]
            lib.cairo_surface_mark_dirty(be.surf)
        c = _group(be, content, n)
        m = _group(be, mask, n)
        lib.cairo_set_source(cr, c)
        lib.cairo_set_operator(cr, operator)
        lib.cairo_mask(cr, m)
        lib.cairo_pattern_destroy(m)
        lib.cairo_pattern_destroy(c)
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


def _triples(rng):
    content = random_premultiplied(rng, N, "translucent")
    content[N // 2: N // 2 + N // 16] = random_premultiplied(rng, N // 16, "opaque")
    mask = random_premultiplied(rng, N, "translucent")
    mask[N // 4: N // 4 + N // 16] = random_premultiplied(rng, N // 16, "opaque")
    mask[-N // 16:] = 0                                      # transparent mask pixels
    content[-N // 8: -N // 16] = 0                           # transparent content pixels under a live mask
    return content, mask


@needs_cairo
@pytest.mark.parametrize("mode", sorted(mk.MODES))
@pytest.mark.parametrize("ground", ["opaque", "translucent", "clear_pixels", "still_clear"])
def test_model_is_libcairo(mode, ground):
    rng = np.random.default_rng(sorted(mk.MODES).index(mode) * 7 + 29)
    content, mask = _triples(rng)
    dst = None if ground == "still_clear" else random_premultiplied(rng, N, "clear" if ground == "clear_pixels" else ground)
    got = _mask(dst, content, mask, bm.CAIRO_OPERATORS[mode], N)
    d = np.zeros((N, 4), np.uint8) if dst is None else dst
    want = mk.composite(mode, content, mask, d)
    bad = np.flatnonzero((got != want).any(-1))
    assert bad.size == 0, "%d of %d pixels differ, first: content %s mask %s dst %s cairo %s model %s" % (
        bad.size, N, content[bad[0]], mask[bad[0]], d[bad[0]], got[bad[0]], want[bad[0]])
    assert (got != d).any(-1).sum() > N // 2                 # (the operator did something)
    assert (got[-N // 16:] == d[-N // 16:]).all()            # a transparent mask pixel leaves the destination as it is
    assert (got[-N // 8:] == d[-N // 8:]).all()              # ... and so does a transparent content pixel


def test_the_masks_colour_plays_no_part_and_transparency_changes_nothing():
    rng = np.random.default_rng(5)
    content, mask = _triples(rng)
    other = mask.copy()
    other[:, :3] = (other[:, 3:4].astype(int) * rng.integers(0, 256, (N, 3)) // 255).astype(np.uint8)
    assert (other[:, :3] != mask[:, :3]).any()
    for kind in ("translucent", "opaque", "clear"):
        d = random_premultiplied(rng, N, kind)
        for mode in mk.MODES:
            assert (mk.composite(mode, content, mask, d) == mk.composite(mode, content, other, d)).all()
            assert (mk.composite(mode, content, np.zeros_like(mask), d) == d).all(), (mode, kind)
            assert (mk.composite(mode, np.zeros_like(content), mask, d) == d).all(), (mode, kind)
    # 0x80 rounding, not 0x7f and not truncation: 1 * 128 / 255 rounds to 1
    assert mk.masked(np.array([[1, 1, 1, 1]], np.uint8), np.array([[0, 0, 0, 128]], np.uint8)).tolist() == [[1, 1, 1, 1]]
    assert mk.masked(np.array([[1, 1, 1, 1]], np.uint8), np.array([[0, 0, 0, 127]], np.uint8)).tolist() == [[0, 0, 0, 0]]


@needs_cairo
@pytest.mark.parametrize("mode", sorted(mk.MODES))
def test_clear_surface_bookkeeping_is_libcairos(mode):
    """On a still-clear parent: the pixels after cairo_mask, and whether libcairo still takes the parent for clear -- seen in a
    translucent fill behind it, a SOURCE lerp on a clear surface (the premultiplied colour itself) and OVER otherwise.  Content and mask
    each still clear, or drawn on with every pixel zero."""
    n = 512
    zero = np.zeros((n, 4), np.uint8)
    probe = (97, 184, 252, 38)             # (0x7f and 0x80 rounding differ at one coverage value per channel value at most: this colour has one)
    lerp = _mask(None, None, None, CAIRO_OPERATOR_OVER, n, probe)[1]          # nothing at all happened to the parent
    over = _mask(random_premultiplied(np.random.default_rng(1), n, "clear"), None, None, CAIRO_OPERATOR_OVER, n, probe)[1]   # a drawn-on parent
    assert (lerp != over).any()                              # (the probe tells the two states apart)
    for content_clear in (True, False):
        for mask_clear in (True, False):
            out, after = _mask(None, None if content_clear else zero, None if mask_clear else zero, bm.CAIRO_OPERATORS[mode], n, probe)
            assert (out == 0).all()
            stays = mk.nothing_to_do(mode, content_clear, mask_clear)
            assert (after == (lerp if stays else over)).all(), (mode, content_clear, mask_clear, stays)
    # a parent that was drawn on stays drawn on
    d = random_premultiplied(np.random.default_rng(2), n, "clear")
    assert (_mask(d, None, None, bm.CAIRO_OPERATORS[mode], n, probe)[1] == over).all()
