"""tests/blend_model.py -- the blend-mode rule in numpy -- against live libcairo, pixel by pixel, and the committed blend goldens
re-rendered by live libcairo.  No GPU.  Skipped where libcairo is absent."""
import ctypes

import numpy as np
import pytest

import blend_model as bm
from cairo_pixels import random_premultiplied, surface_bytes
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
N = 4096                                   # pixels (= random triples) per operator and destination kind


def _paint(dst, colours, widths, operator, mark_dirty=True):
    """pixel i of an n x 1 surface holding `dst` (premultiplied R, G, B, A; None: a cleared surface): the rectangle (i, 0, widths[i], 1)
    filled with colours[i] (straight r, g, b, a) under `operator` -- a box path with coverage ~ widths[i]"""
    n = len(colours)
    be = cb.CairoBackend(n, 1)
    try:
        be.clear_all()
        if dst is not None:
            surface_bytes(be)[0] = dst[:, [2, 1, 0, 3]]
            be.lib.cairo_surface_mark_dirty(be.surf)
        be.lib.cairo_set_operator(be.cr, operator)
        for i in range(n):
            r, g, b, a = (int(v) for v in colours[i])
            be.lib.cairo_set_source_rgba(be.cr, r / 255.0, g / 255.0, b / 255.0, a / 255.0)
            be.lib.cairo_new_path(be.cr)
            be.lib.cairo_rectangle(be.cr, float(i), 0.0, float(widths[i]), 1.0)
            be.lib.cairo_fill(be.cr)
        return be.premultiplied_rgba()[0].copy()
    finally:
        be.close()


def _triples(seed):
    rng = np.random.default_rng(seed)
    colours = rng.integers(0, 256, (N, 4))
    colours[: N // 8, 3] = rng.choice([1, 119, 254, 255], N // 8)
    widths = rng.integers(0, 257, N) / 256.0
    widths[N // 2: N // 2 + N // 8] = 1.0
    widths[widths == 0] = 1.0 / 256
    # the coverage byte of every rectangle: the alpha an opaque white OVER of the same path leaves on a clear surface
    cov = _paint(None, np.full((N, 4), 255), widths, 2)[:, 3]
    return rng, colours, widths, cov


@needs_cairo
@pytest.mark.parametrize("mode", sorted(bm.MODES))
@pytest.mark.parametrize("ground", ["opaque", "translucent", "clear_pixels"])
def test_model_is_libcairo(mode, ground):
    rng, colours, widths, cov = _triples(sorted(bm.MODES).index(mode) * 3 + 11)
    # ("clear_pixels": transparent pixels of a surface that has been drawn on -- not Cairo's "still clear" surface, which is below)
    dst = random_premultiplied(rng, N, "clear" if ground == "clear_pixels" else ground)
    got = _paint(dst, colours, widths, bm.CAIRO_OPERATORS[mode])
    c = bm.source_pixel(colours[:, 0], colours[:, 1], colours[:, 2], colours[:, 3])
    want = bm.blend(mode, c, cov, dst)
    bad = np.flatnonzero((got != want).any(-1))
    assert bad.size == 0, "%d of %d pixels differ, first: src %s cov %d dst %s cairo %s model %s" % (
        bad.size, N, c[bad[0]], cov[bad[0]], dst[bad[0]], got[bad[0]], want[bad[0]])
    assert (got != dst).any(-1).sum() > N // 2               # (the operator did something: the comparison is not of two untouched surfaces)


@needs_cairo
def test_add_on_a_clear_surface_is_source_and_the_others_are_not():
    """the first paint of a frame: ADD becomes the SOURCE lerp (0x7f rounding), as OVER does; the other seven stay themselves"""
    rng, colours, widths, cov = _triples(5)
    c = bm.source_pixel(colours[:, 0], colours[:, 1], colours[:, 2], colours[:, 3])
    zero = np.zeros((1, 4), np.uint8)
    # the triples where the two roundings part (SOURCE: 0x7f, ADD of mul_un8: 0x80) and as many where they agree
    parts = (bm.lerp_source(c, cov, np.zeros_like(c)) != bm.blend("add", c, cov, np.zeros_like(c))).any(-1)
    assert parts.sum() >= 8                                  # (the case distinguishes the two at all)
    picks = list(np.flatnonzero(parts)[:48]) + list(np.flatnonzero(~parts)[:48])
    for k, i in enumerate(picks):                            # (one fill per surface: a surface's second fill is no longer its first)
        got_add = _paint(None, colours[i:i + 1], widths[i:i + 1], bm.CAIRO_OPERATORS["add"])
        want = bm.lerp_source(c[i:i + 1], cov[i:i + 1], zero)
        assert (got_add == want).all(), (c[i], cov[i], got_add, want)
        if k % 4 == 0:
            for other in sorted(set(bm.MODES) - {"add"}):
                got = _paint(None, colours[i:i + 1], widths[i:i + 1], bm.CAIRO_OPERATORS[other])
                assert (got == bm.blend(other, c[i:i + 1], cov[i:i + 1], zero)).all(), other


def test_no_coverage_changes_nothing():
    rng = np.random.default_rng(3)
    d = random_premultiplied(rng, 20000, "translucent")
    c = random_premultiplied(rng, 20000, "translucent")
    for mode in list(bm.MODES) + ["normal"]:
        assert (bm.blend(mode, c, np.zeros(20000, np.int64), d) == d).all(), mode


def test_everything_fits_32_bits():
    """the separable modes' sums stay below 3 * 65025 and never go negative for premultiplied operands"""
    v = np.arange(256)
    sa, da = np.meshgrid(v, v, indexing="ij")
    for s_frac in (0.0, 0.5, 1.0):
        for d_frac in (0.0, 0.5, 1.0):
            s, d = (sa * s_frac).astype(np.int64), (da * d_frac).astype(np.int64)
            over = sa * da - 2 * (da - d) * (sa - s)
            for b in (s * da + d * sa - s * d, np.abs(d * sa - s * da), np.maximum(s * da, d * sa),
                      np.where(2 * d < da, 2 * s * d, over), np.where(2 * s < sa, 2 * s * d, over)):
                t = (255 - sa) * d + (255 - da) * s + b
                assert t.min() >= 0 and t.max() < 3 * 65025


@needs_cairo
def test_committed_goldens_are_what_libcairo_renders():
    import blend_scenes as bs
    checked = 0
    for fname, arrays in bs.goldens().items():
        old = np.load(bs.golden_path(fname))
        assert sorted(old.files) == sorted(arrays)
        for k, v in arrays.items():
            assert old[k].dtype == np.uint8 and (old[k] == v).all(), (fname, k)
            checked += 1
    assert checked > 100
