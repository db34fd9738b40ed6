"""tests/alpha_modes_model.py -- the erase and alpha rule in numpy -- against live libcairo: CAIRO_OPERATOR_DEST_OUT and DEST_IN pixel by
pixel under cairo_paint, cairo_paint_with_alpha and cairo_mask of a group; per-path ERASE fills; the unbounded clearing of a per-path
DEST_IN fill (why alpha per path is refused); libcairo's clear-surface bookkeeping behind the two operators; and the committed
goldens.  No GPU.  Skipped where libcairo is absent."""
import ctypes

import numpy as np
import pytest

import alpha_modes_model as am
import alpha_modes_scenes as scenes
import blend_model as bm
import blend_scenes as bs
import fade_model as fd
import host_frames as hf
import mask_model as mk
from alpha_modes_scenes import CLEAR_FILL, FOLLOW, _faded, _layer, _masked, _pair, _rect, _scene, _shape
from cairo_pixels import random_premultiplied, surface_bytes
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
N = 4096                                   # random pairs per operator, form and ground
OPACITIES = (1, 77, 128, 254)


def _declare(lib):
    P, D = ctypes.c_void_p, ctypes.c_double
    for fn, res, args in (("cairo_push_group", None, [P]), ("cairo_pop_group_to_source", None, [P]), ("cairo_pop_group", P, [P]),
                          ("cairo_get_group_target", P, [P]), ("cairo_paint_with_alpha", None, [P, D]), ("cairo_paint", None, [P]),
                          ("cairo_set_source", None, [P, P]), ("cairo_mask", None, [P, P]), ("cairo_pattern_destroy", None, [P])):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args


def _write_group(lib, cr, pixels, n):
    target = lib.cairo_get_group_target(cr)
    lib.cairo_surface_flush(target)
    stride = lib.cairo_image_surface_get_stride(target)
    data = np.ctypeslib.as_array(lib.cairo_image_surface_get_data(target), shape=(1, stride))
    data[0, : n * 4] = pixels[:, [2, 1, 0, 3]].reshape(-1)
    lib.cairo_surface_mark_dirty(target)


def _composite(dst, group, mode, n, opacity=None, mask=None):
    """an n x 1 surface holding `dst` (None: a cleared surface nothing was drawn on); a group holding `group` composited onto it under
    the mode's operator: cairo_paint, cairo_paint_with_alpha(opacity / 255) or, with `mask` (the pixels of a second group), cairo_mask"""
    be = cb.CairoBackend(n, 1)
    lib, cr = be.lib, be.cr
    _declare(lib)
    try:
        be.clear_all()
        if dst is not None:
            surface_bytes(be)[0] = dst[:, [2, 1, 0, 3]]
            lib.cairo_surface_mark_dirty(be.surf)
        lib.cairo_push_group(cr)
        _write_group(lib, cr, group, n)
        if mask is None:
            lib.cairo_pop_group_to_source(cr)
            lib.cairo_set_operator(cr, am.CAIRO_OPERATORS[mode])
            if opacity is None:
                lib.cairo_paint(cr)
            else:
                lib.cairo_paint_with_alpha(cr, opacity / 255.0)
        else:
            content = lib.cairo_pop_group(cr)
            lib.cairo_push_group(cr)
            _write_group(lib, cr, mask, n)
            mpat = lib.cairo_pop_group(cr)
            lib.cairo_set_source(cr, content)
            lib.cairo_set_operator(cr, am.CAIRO_OPERATORS[mode])
            lib.cairo_mask(cr, mpat)
            lib.cairo_pattern_destroy(mpat)
            lib.cairo_pattern_destroy(content)
        assert lib.cairo_status(cr) == 0
        return be.premultiplied_rgba()[0].copy()
    finally:
        be.close()


def _group(rng, n):
    group = random_premultiplied(rng, n, "translucent")
    group[n // 2: n // 2 + n // 16] = random_premultiplied(rng, n // 16, "opaque")
    group[-n // 16:] = 0
    return group


@needs_cairo
@pytest.mark.parametrize("ground", ["opaque", "translucent", "clear_pixels", "still_clear"])
@pytest.mark.parametrize("form", ["plain", "paint_with_alpha", "mask"])
@pytest.mark.parametrize("mode", ["erase", "alpha"])
def test_the_rule_is_libcairos(mode, form, ground):
    rng = np.random.default_rng(17 + 5 * (mode == "alpha") + len(form) + len(ground))
    group = _group(rng, N)
    dst = None if ground == "still_clear" else random_premultiplied(rng, N, "clear" if ground == "clear_pixels" else ground)
    d = np.zeros((N, 4), np.uint8) if dst is None else dst
    if form == "plain":
        cases = [(_composite(dst, group, mode, N), group)]
    elif form == "paint_with_alpha":
        cases = [(_composite(dst, group, mode, N, opacity=o), fd.faded(group, o)) for o in OPACITIES]
    else:
        mask = _group(np.random.default_rng(99), N)[::-1].copy()
        cases = [(_composite(dst, group, mode, N, mask=mask), mk.masked(group, mask))]
    for got, s in cases:
        want = am.combine(mode, s, d)
        bad = np.argwhere((got != want).any(-1))
        assert len(bad) == 0, "%d of %d pixels differ, first: source %s dst %s cairo %s model %s" % (len(bad), N, s[bad[0][0]], d[bad[0][0]], got[bad[0][0]], want[bad[0][0]])
        if ground in ("opaque", "translucent"):
            assert (got != d).any()                          # (the operator did something)
            # a transparent source pixel: ERASE leaves the destination as it is, ALPHA clears it
            assert (got[-N // 16:] == (d[-N // 16:] if mode == "erase" else 0)).all()


def test_the_rule_in_numbers():
    d = np.array([[200, 100, 50, 255]], np.uint8)
    s = np.array([[9, 9, 9, 128]], np.uint8)
    assert am.combine("erase", s, d).tolist() == [[100, 50, 25, 127]] and am.combine("alpha", s, d).tolist() == [[100, 50, 25, 128]]
    z = np.zeros((1, 4), np.uint8)
    assert (am.combine("erase", z, d) == d).all() and (am.combine("alpha", z, d) == 0).all()
    full = np.array([[1, 2, 3, 255]], np.uint8)
    assert (am.combine("erase", full, d) == 0).all() and (am.combine("alpha", full, d) == d).all()
    # 0x80 rounding, not 0x7f, not truncation
    one = np.array([[1, 1, 1, 1]], np.uint8)
    assert am.combine("alpha", np.array([[0, 0, 0, 128]], np.uint8), one).tolist() == [[1, 1, 1, 1]]
    assert am.combine("alpha", np.array([[0, 0, 0, 127]], np.uint8), one).tolist() == [[0, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------------------------- per path
def _path_scene(aliased_unused, ground, colour):
    kids = [_shape([(5.3, 3.2), (58.6, 12.7), (20.2, 40.4)], colour), _rect(30.37, 20.21, 55.62, 41.45, colour), _rect(8, 30, 28, 44, colour)]
    return _scene(bs._grounds(64, 48)[ground] + [{"type": "container", "blend_mode": "erase", "children": kids}])


@needs_cairo
@pytest.mark.parametrize("aliased", [False, True], ids=["antialiased", "aliased"])
def test_per_path_erase_fills_are_libcairos(aliased):
    """a triangle, an off-grid box and an on-grid box in opaque, alpha-100 and alpha-1 colours over an opaque and a translucent ground:
    libcairo's pixels, the frame builder's arrays through the numpy renderer"""
    for ground in ("opaque", "translucent"):
        for colour in ((230, 40, 90, 255), (40, 200, 120, 100), (20, 60, 240, 1)):
            sc = _path_scene(aliased, ground, colour)
            want = scenes.cairo_render(sc, aliased)
            e, p, s = scenes.build_flagged(sc, aliased)
            assert [int(v) for v in p["lerp"]][1:] == [am.OP_ERASE << 8] * 3
            got = am.render(e, p, s, 64, 48, aliased=aliased)
            assert (got == want).all(), (ground, colour, int((got != want).any(-1).sum()))
            plain = scenes.cairo_render(_scene(bs._grounds(64, 48)[ground]), aliased)
            assert (want != plain).any() and (want[..., 3] <= plain[..., 3]).all()         # erase only ever takes away


@needs_cairo
def test_a_per_path_dest_in_fill_clears_the_surface_outside_the_path():
    """why "alpha" stays refused as a per-path blend mode: DEST_IN is unbounded, one fill clears every pixel outside its path"""
    be = cb.CairoBackend(64, 48)
    lib, cr = be.lib, be.cr
    try:
        be.clear_all()
        lib.cairo_set_source_rgba(cr, 0.2, 0.4, 0.9, 0.8)
        lib.cairo_rectangle.argtypes = [ctypes.c_void_p] + [ctypes.c_double] * 4
        lib.cairo_rectangle(cr, 0, 0, 64, 48)
        lib.cairo_fill(cr)
        before = be.premultiplied_rgba().copy()
        assert before[..., 3].all()
        lib.cairo_set_operator(cr, am.CAIRO_OPERATORS["alpha"])
        lib.cairo_set_source_rgba(cr, 1, 0, 0, 1)
        lib.cairo_move_to(cr, 10, 10)
        lib.cairo_line_to(cr, 30, 12)
        lib.cairo_line_to(cr, 18, 30)
        lib.cairo_fill(cr)
        after = be.premultiplied_rgba().copy()
    finally:
        be.close()
    outside = np.ones((48, 64), bool)
    outside[10:30, 10:30] = False
    assert not after[outside].any() and int(outside.sum()) > 2500      # every pixel outside the path's extents is gone
    assert after[12:28, 12:28].any() and (after[15, 17] == before[15, 17]).all()
    # the same fill under DEST_OUT changes nothing outside the path
    sc = _scene([_rect(0, 0, 64, 48, (51, 102, 230, 204)), dict(_shape([(10, 10), (30, 12), (18, 30)], (255, 0, 0, 255)), blend_mode="erase")])
    erased = scenes.cairo_render(sc)
    ground = scenes.cairo_render(_scene([_rect(0, 0, 64, 48, (51, 102, 230, 204))]))
    assert (erased[outside] == ground[outside]).all() and (erased != ground).any()


# ---------------------------------------------------------------------------------------------------------------- the clear state
BIG = [(20.4, 11.3), (280.2, 60.1), (90.6, 190.3)]                   # a 300 x 200 triangle


def _prelude(name):
    tri = _shape([(30, 20), (200, 40), (100, 150)], (200, 30, 60, 180))
    return {"erase_path": [dict(tri, blend_mode="erase")], "erase_layer": [_layer("erase", [tri])], "alpha_layer": [_layer("alpha", [tri])],
            "alpha_empty": [_layer("alpha", [])], "paint_erase_all": [_rect(0, 0, 300, 200, (9, 99, 199, 255)), dict(_rect(0, 0, 300, 200, (0, 0, 0, 255)), blend_mode="erase")],
            "erase_clear_source": [dict(_shape([(30, 20), (200, 40), (100, 150)], (255, 255, 255, 0)), blend_mode="erase")]}[name]


@needs_cairo
@pytest.mark.parametrize("name", ["erase_path", "erase_layer", "alpha_layer", "alpha_empty", "paint_erase_all", "erase_clear_source"])
def test_the_operators_end_the_still_clear_state(name):
    """each prelude changes no pixel of a clear 300 x 200 surface, yet the translucent triangle behind it is composited with OVER, not
    with the SOURCE lerp of a first paint: libcairo's pixels are the frame builder's arrays through the numpy renderer, and they are
    NOT what the same arrays give with the triangle's lerp bit set"""
    rng = np.random.default_rng(12)
    differing = 0
    for k in range(4):
        colour = tuple(int(v) for v in rng.integers(0, 256, 3)) + (100 + k,)
        sc = _scene(_prelude(name) + [_shape(BIG, colour)], 300, 200)
        want = scenes.cairo_render(sc)
        e, p, s = scenes.build_flagged(sc)
        assert int(p["lerp"][-1]) == 0 and int(p["kind"][-1]) == 0, name
        over = am.render(e, p, s, 300, 200)
        assert (over == want).all(), (name, colour, int((over != want).any(-1).sum()))
        q = p.copy()
        q["lerp"][-1] = 1
        lerp = am.render(e, q, s, 300, 200)
        differing += int((lerp != over).any(-1).sum())
        fresh = scenes.cairo_render(_scene([_shape(BIG, colour)], 300, 200))
        assert (fresh == lerp).all()                                 # (on a fresh surface the triangle IS the lerp)
    assert differing > 0, "the two candidate rules agree on this input: the test shows nothing"


@needs_cairo
def test_what_returns_at_once_leaves_the_surface_clear():
    """an ERASE layer at opacity 0 and one masked by an untouched mask return at once in libcairo (DEST_OUT is bounded by its mask):
    the triangle behind them is still a first paint"""
    colour = (31, 164, 79, 101)
    fresh = scenes.cairo_render(_scene([_shape(BIG, colour)], 300, 200))
    for prelude in ([_faded("erase", 0, _pair())], [_masked("erase", _pair(), [])]):
        sc = _scene(prelude + [_shape(BIG, colour)], 300, 200)
        assert (scenes.cairo_render(sc) == fresh).all()
        e, p, s = scenes.build_flagged(sc)
        assert [int(v) for v in p["lerp"]] == [1]
        assert (am.render(e, p, s, 300, 200) == fresh).all()


# ---------------------------------------------------------------------------------------------------------------- the goldens
@needs_cairo
@pytest.mark.parametrize("fname", sorted(scenes.files()))
def test_the_committed_goldens_are_what_libcairo_renders(fname):
    make, aliased = scenes.files()[fname]
    gold = np.load(scenes.golden_path(fname))
    items = sorted(make().items())
    assert [n for n, _ in items] == sorted(gold.files)
    for name, sc in items:
        assert (scenes.cairo_render(sc, aliased) == gold[name]).all(), (fname, name)


def test_the_goldens_show_the_feature():
    """alpha clears the ground outside the layer, erase leaves it; the golden files are small"""
    import os
    gold = np.load(scenes.golden_path("cairo_alphamode_layers"))
    a, e = gold["layer_alpha_opaque"], gold["layer_erase_opaque"]
    assert ((a[..., 3] == 0) & (e[..., 3] == 255)).sum() > 200          # the ground beside the layer's children: gone, and untouched
    assert ((a[..., 3] > 0) & (e[..., 3] == 255)).sum() == 0            # what alpha keeps lies under the children, where erase took away
    for fname in scenes.files():
        assert os.path.getsize(scenes.golden_path(fname)) < 200 * 1024
