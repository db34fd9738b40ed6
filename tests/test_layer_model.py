"""tests/layer_model.py -- the isolated-layer rule in numpy -- against live libcairo, pixel by pixel (a real cairo_push_group /
cairo_pop_group_to_source / cairo_paint), and the committed layer goldens re-rendered by live libcairo.  No GPU.  Skipped where libcairo
is absent."""
import ctypes

import numpy as np
import pytest

import blend_model as bm
from cairo_pixels import random_premultiplied, surface_bytes
import layer_model as lm
from oracle import cairo_backend as cb

needs_cairo = pytest.mark.skipif(not cb.available(), reason="libcairo not installed")
N = 4096                                   # pixels (= random pairs) per operator and destination kind


def _composite(dst, group, operator):
    """an n x 1 surface holding `dst` (premultiplied R, G, B, A; None: a cleared surface nothing was drawn on), a group holding `group`
    painted onto it under `operator`"""
    n = len(group)
    be = cb.CairoBackend(n, 1)
    lib, cr = be.lib, be.cr
    for fn, res in (("cairo_push_group", None), ("cairo_pop_group_to_source", None), ("cairo_paint", None), ("cairo_get_group_target", ctypes.c_void_p)):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, [ctypes.c_void_p]
    try:
        be.clear_all()
        if dst is not None:
            surface_bytes(be)[0] = dst[:, [2, 1, 0, 3]]
            lib.cairo_surface_mark_dirty(be.surf)
        lib.cairo_push_group(cr)
        target = lib.cairo_get_group_target(cr)
        lib.cairo_surface_flush(target)
        stride = lib.cairo_image_surface_get_stride(target)
        data = np.ctypeslib.as_array(lib.cairo_image_surface_get_data(target), shape=(1, stride))
        data[0, : n * 4] = group[:, [2, 1, 0, 3]].reshape(-1)
        lib.cairo_surface_mark_dirty(target)
        lib.cairo_pop_group_to_source(cr)
        lib.cairo_set_operator(cr, operator)
        lib.cairo_paint(cr)
        assert lib.cairo_status(cr) == 0
        return be.premultiplied_rgba()[0].copy()
    finally:
        be.close()


@needs_cairo
@pytest.mark.parametrize("mode", sorted(lm.MODES))
@pytest.mark.parametrize("ground", ["opaque", "translucent", "clear_pixels", "still_clear"])
def test_model_is_libcairo(mode, ground):
    rng = np.random.default_rng(sorted(lm.MODES).index(mode) * 5 + 17)
    group = random_premultiplied(rng, N, "translucent")
    group[N // 2: N // 2 + N // 16] = random_premultiplied(rng, N // 16, "opaque")
    group[-N // 16:] = 0
    # ("clear_pixels": transparent pixels of a surface that has been drawn on; "still_clear": Cairo's still-clear surface)
    dst = None if ground == "still_clear" else random_premultiplied(rng, N, "clear" if ground == "clear_pixels" else ground)
    got = _composite(dst, group, bm.CAIRO_OPERATORS[mode])
    d = np.zeros((N, 4), np.uint8) if dst is None else dst
    want = lm.composite(mode, group, d)
    bad = np.flatnonzero((got != want).any(-1))
    assert bad.size == 0, "%d of %d pixels differ, first: group %s dst %s cairo %s model %s" % (
        bad.size, N, group[bad[0]], d[bad[0]], got[bad[0]], want[bad[0]])
    assert (got != d).any(-1).sum() > N // 2                 # (the operator did something)
    assert (got[-N // 16:] == d[-N // 16:]).all()            # a transparent group pixel leaves the destination as it is


def test_a_transparent_group_pixel_changes_nothing():
    rng = np.random.default_rng(3)
    for kind in ("translucent", "opaque", "clear"):
        d = random_premultiplied(rng, 20000, kind)
        for mode in lm.MODES:
            assert (lm.composite(mode, np.zeros_like(d), d) == d).all(), (mode, kind)


def test_unmasked_is_coverage_255():
    v = np.arange(256)
    assert (bm.mul_un8(v, 255) == v).all()


@needs_cairo
def test_committed_goldens_are_what_libcairo_renders():
    import layer_scenes as ls
    checked = 0
    for fname, arrays in ls.goldens().items():
        old = np.load(ls.golden_path(fname))
        assert sorted(old.files) == sorted(arrays)
        for k, v in arrays.items():
            assert old[k].dtype == np.uint8 and (old[k] == v).all(), (fname, k)
            checked += 1
    assert checked > 100


@needs_cairo
def test_bookkeeping_scenes_discriminate():
    """every clear-state scene follows layer_model.parent_stays_clear and differs from the other rule in at least one pixel; a single
    path in an OVER layer differs from the plain path (tools/make_composite_goldens.py checks the same before it writes)"""
    import layer_scenes as ls
    scenes = ls.structure_scenes()
    wrong = ls.wrong_rule_scenes()
    assert len(wrong) == len(ls.CLEAR_STATE) * len(ls.MODES) + 3
    for name, (right, other) in sorted(wrong.items()):
        want = ls.cairo_render(scenes[name])
        for sc, same in ((right, True), (other, False)):
            if sc is None:
                continue
            img = ls.cairo_render(sc)
            if sc.get("speck"):
                img[47, 63] = want[47, 63]
            assert bool((img == want).all()) == same, (name, same)
    for name in wrong:
        kind, mode = name.rsplit("_", 1)
        if kind in ls.CLEAR_STATE:
            stays = lm.parent_stays_clear(mode, kind != "clear_fill_multiply")
            assert ("speck" in wrong[name][1]) == stays, name      # (the wrong rule is "drawn" exactly where the model says "stays clear")
