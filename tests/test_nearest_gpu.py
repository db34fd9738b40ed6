"""Unsmoothed bitmap fills on the device (raster2.hip: bilinear_taps_at behind shade_bitmap and the transposed fetch of blend8 -- its
wave-uniform "strictly inside" path and the general routine -- which every k2_tiles instance from 1 up samples through).

Every libcairo golden of tests/nearest_scenes.py's files() -- the three edge rules magnified, 1:1, minified and rotated, the texel-edge
fills, bitmaps a texel wide and high, an 80 x 24 bitmap that holds whole wavefronts, under "blend_mode", "layer", "mask" and
"opacity", antialiased and aliased -- through render (also with the instance forced to 1), swfr_render_edges (+ resident frames),
SWFR_GRAPHS=1, two-band handles (contiguous and interleaved) and render_batch with unlike frames; the colour-transformed scenes
(cxform_files(): variant textures, which belong to the handle that walked the stage) through the same five routes the way
tests/test_pad_gpu.py takes them; the structure and cxform scenes once through each of the instances 2 to 6.  Then 96 random boxes per
edge rule against tests/nearest_model.py in one render_batch, and a frame without the key against the same frame with filter 0.  Zero
differing bytes everywhere.

The oracle knows nothing of the filter.  On a library without the feature the key is ignored and the fills come out bilinear (or
convolved): the golden and the model comparisons fail.

Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import numpy as np
import pytest

import device_routes as dr
import nearest_model as nm
import nearest_scenes as ns
from device_routes import EMU, renderer_for
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)

pytestmark = pytest.mark.gpu
FAMILY = dr.Family("nearest", ns, "1", True, (True, False))
FILES = sorted(ns.files())


class _CxformScenes:
    """the scenes module as device_routes sees it, files() being the colour-transformed ones"""
    files = staticmethod(ns.cxform_files)
    golden_path = staticmethod(ns.golden_path)
    LINEAR_BOUND = ns.LINEAR_BOUND


CXFORM_FAMILY = dr.Family("nearest_cxform", _CxformScenes, "1", True, (True, False))
CXFORM_FILES = sorted(ns.cxform_files())


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
    assert any(st.kind == api.STYLE_BITMAP and st.bitmap >= api.VARIANT_BASE and st.filter == 1 for st in s), "no nearest variant texture in the frame"
    return r, (e, p, s)


@pytest.mark.parametrize("fname", CXFORM_FILES)
def test_cxform_goldens_through_render_edges(fname):
    """swfr_build_frame and swfr_render_edges on ONE handle, then resident frames: the nearest variant textures from uploaded arrays"""
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
    """the heavier instances sample through the same routines: the structure, edges and cxform files (every fourth scene on the
    emulator) forced through each"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    for fname, make in (("cairo_nearest_structure", ns.structure_scenes), ("cairo_nearest_edges", ns.edge_scenes), ("cairo_nearest_cxform", ns.cxform_scenes)):
        gold = np.load(ns.golden_path(fname))
        for name, sc in sorted(make().items())[int(instance) % 4 if EMU else 0:: 4 if EMU else 1]:
            r = renderer_for(sc, False)
            try:
                r.render(sc["stage"])
                dr.check(FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "instance", instance))
                dr.not_refused(r, name)
            finally:
                r.close()


@pytest.mark.parametrize("extend", ns.EXTENDS)
def test_random_boxes_against_the_model(extend):
    """96 random single boxes on a clear 32 x 16 frame (tests/nearest_scenes.py, random_box_case -- the boxes tests/test_nearest_model.py
    holds against libcairo), texels registered as straight RGBA with translucent ones among them, in ONE render_batch on one handle:
    every frame is the model's source samples"""
    rng = np.random.default_rng(4300 + len(extend))
    n = 24 if EMU else 96
    cases = [ns.random_box_case(rng, extend, minified=bool(it & 1)) for it in range(n)]
    want = [nm.frame(c["model"]["matrices"], nm.premultiply(c["model"]["bitmap"]), c["model"]["rect"], {"none": nm.NONE, "repeat": nm.REPEAT, "pad": nm.PAD}[extend], ns.FW, ns.FH)[0]
            for c in cases]
    r = dr.handle(ns.FW, ns.FH)
    try:
        stages = []
        for k, c in enumerate(cases):                                # every box its own bitmap id on the one handle
            (w, h, px), = c["scene"]["raw_bitmaps"].values()
            r.register_bitmap(100 + k, w, h, px)
            stage = ns.with_filter(c["scene"]["stage"], "nearest")
            stage["children"][0]["definition"]["shape"]["initial_styles"]["fill"][0]["bitmap_id"] = 100 + k
            stages.append(stage)
        if EMU:
            got = []
            for stage in stages:
                r.render(stage)
                got.append(r.read_image(premultiplied=True).copy())
        else:
            import torch
            out = torch.zeros((n, ns.FH, ns.FW, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), ns.FH * ns.FW * 4)
            got = out.cpu().numpy()
        dr.not_refused(r, extend)
    finally:
        r.close()
    bad = 0
    for k, c in enumerate(cases):
        d = int((got[k] != want[k]).sum())
        if d:
            bad += 1
            print("case", k, extend, c["aim"], c["model"]["matrices"], c["model"]["rect"], c["model"]["bitmap"].shape, "differing bytes", d)
    assert bad == 0, "%d of %d %s boxes differ from the model" % (bad, n, extend)


def test_an_absent_key_is_filter_0():
    """a frame with good fills of all three edge rules, magnified and minified: the key absent, "good" and 0 give the same bytes (and
    "nearest" other ones)"""
    scenes = [ns.shape_scenes()["nearest_beside_good_%s" % e] for e in ns.EXTENDS] + [ns.extend_scenes(e)["minified_045"] for e in ns.EXTENDS]
    for sc in scenes[::3 if EMU else 1]:
        frames = {}
        for value in (None, "good", 0, "nearest"):
            r = renderer_for(sc, False)
            try:
                r.render(ns.with_filter(sc["stage"], value))
                frames[value] = r.read_image(premultiplied=True).copy()
            finally:
                r.close()
        assert (frames[None] == frames["good"]).all() and (frames[None] == frames[0]).all()
        assert (frames[None] != frames["nearest"]).any()
