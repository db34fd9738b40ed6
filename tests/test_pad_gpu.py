"""Padded bitmap fills on the device (raster2.hip, bilinear_taps_at and shade_bitmap: every k2_tiles instance from 1 up samples
through them).

Every libcairo golden of tests/pad_scenes.py's files() -- shapes that fit their bitmap and shapes that reach past it, rotated, skewed,
minified, under "blend_mode", "layer", "mask" and "opacity", antialiased and aliased -- through render (also with the instance forced
to 1), swfr_render_edges (+ resident frames), SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with
unlike frames; the colour-transformed scenes (cxform_files(): variant textures, which belong to the handle that walked the stage)
through the same five routes, the arrays of swfr_render_edges and of the graphs route built on the drawing handle itself; the
structure and cxform scenes once through each of the instances 2 to 6.  Then 200 random single boxes against tests/pad_model.py.  Zero differing bytes everywhere.

The oracle knows nothing of pad, so nothing here is held against it bar the plain frames of the batch route.  On a library without
the feature every golden comparison fails: the generator's gate makes sure each golden differs from what the same scene gives
with EXTEND_NONE and with EXTEND_REPEAT.

Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import numpy as np
import pytest

import device_routes as dr
import pad_model as pm
import pad_scenes as ps
from device_routes import EMU, renderer_for
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)

pytestmark = pytest.mark.gpu
FAMILY = dr.Family("pad", ps, "1", True, (True, False))
FILES = sorted(ps.files())


class _CxformScenes:
    """the scenes module as device_routes sees it, files() being the colour-transformed ones"""
    files = staticmethod(ps.cxform_files)
    golden_path = staticmethod(ps.golden_path)
    LINEAR_BOUND = ps.LINEAR_BOUND


CXFORM_FAMILY = dr.Family("pad_cxform", _CxformScenes, "1", True, (True, False))
CXFORM_FILES = sorted(ps.cxform_files())


@pytest.mark.parametrize("forced", [False, True], ids=["picked", "forced"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render(fname, forced, monkeypatch):
    dr.goldens_through_render(FAMILY, fname, monkeypatch, forced)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_edges(fname):
    dr.goldens_through_render_edges(FAMILY, fname)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_with_graphs(fname, monkeypatch):
    dr.goldens_with_graphs(FAMILY, fname, monkeypatch)


@pytest.mark.parametrize("contiguous", FAMILY.layouts, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_two_band_handles(fname, contiguous):
    dr.goldens_through_two_band_handles(FAMILY, fname, contiguous)


@pytest.mark.parametrize("fname", FILES)
def test_goldens_through_render_batch_with_unlike_frames(fname):
    dr.goldens_through_render_batch_with_unlike_frames(FAMILY, fname)


@pytest.mark.parametrize("forced", [False, True], ids=["picked", "forced"])
@pytest.mark.parametrize("fname", CXFORM_FILES)
def test_cxform_goldens_through_render(fname, forced, monkeypatch):
    dr.goldens_through_render(CXFORM_FAMILY, fname, monkeypatch, forced)


def _cxform_arrays_on_the_drawing_handle(sc, aliased):
    """(handle, swfr_build_frame's arrays) -- built on the handle that is going to draw them, which owns the variant textures they name"""
    from swf_renderer_amd import api
    r = renderer_for(sc, aliased)
    e, p, s = r.build_frame(sc["stage"])
    assert any(st.kind == api.STYLE_BITMAP and st.bitmap >= api.VARIANT_BASE and st.extend == 2 for st in s), "no padded variant texture in the frame"
    return r, (e, p, s)


@pytest.mark.parametrize("fname", CXFORM_FILES)
def test_cxform_goldens_through_render_edges(fname):
    """swfr_build_frame and swfr_render_edges on ONE handle, then resident frames: the padded variant textures from uploaded arrays"""
    items, aliased, gold = dr.golden_scenes(CXFORM_FAMILY, fname, 0, thin=False)
    for name, sc in items:
        r, arrays = _cxform_arrays_on_the_drawing_handle(sc, aliased)
        try:
            r.render_edges(*arrays)
            dr.check(CXFORM_FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "render_edges"))
            r.render_resident(3)
            dr.check(CXFORM_FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "resident"))
            dr.not_refused(r, name)
        finally:
            r.close()


@pytest.mark.parametrize("fname", CXFORM_FILES)
def test_cxform_goldens_with_graphs(fname, monkeypatch):
    monkeypatch.setenv("SWFR_GRAPHS", "1")
    items, aliased, gold = dr.golden_scenes(CXFORM_FAMILY, fname, 1, thin=False)
    for name, sc in items:
        r, arrays = _cxform_arrays_on_the_drawing_handle(sc, aliased)
        try:
            r.upload_edges(*arrays)
            r.render_resident(3)
            dr.check(CXFORM_FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "graphs"))
            dr.not_refused(r, name)
        finally:
            r.close()


@pytest.mark.parametrize("contiguous", CXFORM_FAMILY.layouts, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("fname", CXFORM_FILES)
def test_cxform_goldens_through_two_band_handles(fname, contiguous):
    dr.goldens_through_two_band_handles(CXFORM_FAMILY, fname, contiguous)


@pytest.mark.parametrize("fname", CXFORM_FILES)
def test_cxform_goldens_through_render_batch_with_unlike_frames(fname):
    dr.goldens_through_render_batch_with_unlike_frames(CXFORM_FAMILY, fname)


@pytest.mark.parametrize("instance", ["2", "3", "4", "5", "6"])
def test_compositing_scenes_through_instance(instance, monkeypatch):
    """the heavier instances sample through the same routines: the structure and cxform files (every fourth scene on the emulator)
    forced through each"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    for fname, make in (("cairo_pad_structure", ps.structure_scenes), ("cairo_pad_cxform", ps.cxform_scenes)):
        gold = np.load(ps.golden_path(fname))
        for name, sc in sorted(make().items())[int(instance) % 4 if EMU else 0:: 4 if EMU else 1]:
            r = renderer_for(sc, False)
            try:
                r.render(sc["stage"])
                dr.check(FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "instance", instance))
                dr.not_refused(r, name)
            finally:
                r.close()


def test_pad_is_visible():
    """every padded golden differs from what the same scene gives with either of the other two edge rules on the device"""
    gold = np.load(ps.golden_path("cairo_pad_reach"))
    for name, sc in sorted(ps.reach_scenes().items())[::4 if EMU else 1]:
        for extend in ("none", "repeat"):
            r = renderer_for(sc, False)
            try:
                r.render(ps.with_extend(sc["stage"], extend))
                assert (r.read_image(premultiplied=True) != gold[name]).any(), (name, extend)
            finally:
                r.close()


def test_random_boxes_against_the_model():
    """200 random single boxes on a clear 32 x 16 frame (tests/pad_scenes.py, random_box_case -- the boxes tests/test_pad_model.py holds
    against libcairo), texels registered as straight RGBA with translucent ones among them: the frame is the model's source samples"""
    rng = np.random.default_rng(4242)
    seen = {}
    for it in range(24 if EMU else 200):
        case = ps.random_box_case(rng, minified=bool(it & 1))
        sc, md = case["scene"], case["model"]
        src = pm.source(md["matrices"], pm.premultiply(md["bitmap"]), md["rect"])
        want = np.zeros((ps.FH, ps.FW, 4), np.uint8)
        x0, y0, x1, y1 = md["rect"]
        want[y0:y1, x0:x1] = pm.rgba_bytes(src["pixels"])
        r = dr.handle(ps.FW, ps.FH)
        try:
            for bid, (w, h, px) in sc["raw_bitmaps"].items():
                r.register_bitmap(bid, w, h, px)
            r.render(sc["stage"])
            got = r.read_image(premultiplied=True)
            dr.not_refused(r, it)
        finally:
            r.close()
        n = int((got != want).sum())
        assert n == 0, (it, case["aim"], md["matrices"], md["rect"], md["bitmap"].shape, "differing bytes", n)
        seen[case["aim"], src["bilinear"]] = seen.get((case["aim"], src["bilinear"]), 0) + 1
    print("pad boxes", seen)
    assert len(seen) == 6
