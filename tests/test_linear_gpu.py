"""Pixman-exact linear gradients on the device (raster_common.hip, shade_linear; raster2.hip, k2_linear_pieces).

Every libcairo golden of tests/linear_scenes.py -- padded, reflected and repeated linear gradients under horizontal, vertical, rotated
and sheared matrices, polygons, boxes, a concave shape, compositing -- on linear="pixman" handles through render (also with instance 2
forced), swfr_build_frame + swfr_render_edges (+ resident frames), SWFR_GRAPHS=1, two band handles in both layouts and render_batch
with unlike frames; the compositing scenes once through each of the instances 3 to 6.  Zero differing bytes, no LINEAR_BOUND.  And the
default: a linear="float64" handle still renders gradient_linear_ext to the oracle's float64 model.

Without the feature Renderer(linear=...) is a TypeError.  Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import functools

import numpy as np
import pytest

import device_routes as dr
import host_frames
import linear_scenes as ls
from device_routes import EMU
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats, oracle_render

pytestmark = pytest.mark.gpu
FAMILY = dr.Family("linear", ls, "2", True, (True, False))
FILES = sorted(ls.files())


@pytest.fixture(autouse=True)
def pixman_handles(monkeypatch):
    """every handle the routes make -- device and host-only -- is a linear="pixman" one"""
    monkeypatch.setattr(dr, "handle", functools.partial(dr.handle, linear="pixman"))
    monkeypatch.setattr(host_frames, "host", functools.partial(host_frames.host, linear="pixman"))


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


@pytest.mark.parametrize("instance", ["3", "4", "5", "6"])
@pytest.mark.parametrize("spread", ls.SPREADS)
def test_structure_through_instance(spread, instance, monkeypatch):
    """the heavier instances shade through the same call: the compositing scenes forced through each"""
    monkeypatch.setenv("SWFR_TILES_SHADERS", instance)
    fname = "cairo_linear_%s_structure" % spread
    gold = np.load(ls.golden_path(fname))
    for name, sc in sorted(ls.structure_scenes(spread).items())[int(instance) % 2 if EMU else 0:: 2 if EMU else 1]:
        r = dr.renderer_for(sc, False)
        try:
            r.render(sc["stage"])
            dr.check(FAMILY, r.read_image(premultiplied=True), gold[name], sc, (fname, name, "instance", instance))
            dr.not_refused(r, name)
        finally:
            r.close()


def test_the_default_handle_is_the_float64_model():
    """linear="float64", the default: gradient_linear_ext is the oracle's float64 model, as before, within the old bound of 1"""
    import swf_renderer_amd as S
    from scenarios import scenarios
    sc = scenarios()["gradient_linear_ext"]
    want = oracle_render(sc)
    for kw in ({}, {"linear": "float64"}):
        r = S.Renderer(sc["width"], sc["height"], **kw)
        try:
            r.render(sc["stage"])
            n, mx = diff_stats(r.read_image(premultiplied=True), want)
            print("linear default", kw, "differing pixels", n, "max", mx)
            assert mx <= 1
        finally:
            r.close()


def test_a_batch_of_frames_with_unlike_gradient_tables():
    """render_batch launches k2_linear_pieces once for a group of frames, sized for the frame with the most gradient records: a frame
    with fewer -- here a tall frame of many solid paths and no gradient at all, whose scene tables lie where a longer gradient table
    would -- must be left alone, and every frame of the batch must be what the same stage gives on its own"""
    import blend_scenes as bs
    W, H = 130, 400
    lin = lambda spread, dy: ls.ss._scene([ls.ss._shape([(5.3 + k, dy + 1.4 + 3 * k) for k in (0,)] + [(127.6, dy + 2.7), (125.9, dy + 77.3), (6.2, dy + 76.1)],
                                                       ls.fill("rotated", ls.STOPS["ends"], spread, cy=dy + 39.2))], W, H)
    solids = ls.ss._scene([bs._shape([(3.1 + 2 * k, 2.2 + 19 * k), (120.4 - k, 4.6 + 19 * k), (117.2, 17.9 + 19 * k), (4.8, 15.3 + 19 * k)], (30 + 10 * k, 200 - 9 * k, 90, 255 - 7 * k))
                           for k in range(20)], W, H)
    two = ls.ss._scene(lin("reflect", 20)["stage"]["children"] + lin("repeat", 200)["stage"]["children"], W, H)
    frames = [lin("reflect", 10), solids, two, solids, lin("pad", 300)]
    alone = [dr.through_render(sc, linear="pixman") for sc in frames]
    assert (alone[1] == oracle_render(solids)).all()
    r = dr.handle(W, H)
    try:
        stages = [sc["stage"] for sc in frames]
        if EMU:                                                      # (the emulator's device memory is the host's: the grouped route into an array)
            got = np.zeros((len(stages), H, W, 4), np.uint8)
            r.render_batch(stages, got.ctypes.data, H * W * 4)
        else:
            import torch
            out = torch.zeros((len(stages), H, W, 4), dtype=torch.uint8, device="cuda")
            r.render_batch(stages, out.data_ptr(), H * W * 4)
            got = out.cpu().numpy()
        for k in range(len(frames)):
            dr.zero(got[k], alone[k], ("unlike batch", k))
        for cut in (2, 3, 5):
            r.render_batch(stages[:cut])
            dr.zero(r.read_image(premultiplied=True), alone[cut - 1], ("unlike batch, per-frame route", cut))
        dr.not_refused(r, "unlike batch")
    finally:
        r.close()
