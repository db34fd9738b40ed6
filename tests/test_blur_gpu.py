"""Blurred layers on the device ("Blurred layers").

1. the kernels alone: a frame is rendered, captured as a bitmap, blurred, drawn 1:1 with a nearest fill and read back -- against
   tests/blur_model.py (itself held against pixman 0.40 by tests/test_blur_model.py) on the first frame's pixels, zero differing bytes;
2. a 1 x 1 box is the plain layer: the scenes of the existing layer goldens with "layer" turned into "blur", byte for byte;
3. every cairo_blur_* golden (libcairo + pixman) through render, zero differing bytes;
4. the routes that do not draw blurred layers refuse by name, and the handle renders correctly afterwards;
5. a frame without "blur" behind a blurred one is the frame a fresh handle renders.
Runs on an MI355X (-m gpu) and under tools/emu/run.py.
"""
import numpy as np
import pytest

import blur_model as bm
import blur_scenes as bl
import device_routes as dr
import layer_scenes as ls
from device_routes import need_gpu  # noqa: F401 (the module's autouse fixture)
from helpers import diff_stats
from swf_renderer_amd import api

pytestmark = pytest.mark.gpu

FAMILY = dr.FAMILIES["blur"]
SIZES = dr.SIZES
# every width of 1, 2, 3, 4, 64, 255 on either axis
BOX_PAIRS = ((1, 2), (2, 1), (3, 4), (4, 3), (64, 255), (255, 64))
PASSES = (1, 3)
BITMAP = 7


def _content(w, h):
    """translucent and opaque shapes all over a w x h frame, some across its edges (more and larger ones than device_routes.content: the
    blur's own recipe, which leaves few clear pixels)"""
    rng = np.random.default_rng(w * 1000 + h)
    kids = []
    for i in range(24):
        cx, cy = rng.uniform(-0.1, 1.1) * w, rng.uniform(-0.1, 1.1) * h
        pts = [(cx + rng.uniform(-0.35, 0.35) * w, cy + rng.uniform(-0.6, 0.6) * h) for _ in range(3)]
        a = 255 if i % 5 == 0 else int(rng.integers(30, 250))
        kids.append(bl._shape(pts, (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), a)))
    kids.append(bl._rect(0, 0, 1, h / 2, (255, 255, 255, 255)))                  # opaque white against the left edge
    return kids


_whole_frame_bitmap = dr.whole_frame_bitmap


# ---- 1. the kernels alone
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_capture_and_blur_against_the_model(size):
    w, h = size
    r = dr.handle(w, h)
    try:
        with pytest.raises(api.SwfrError) as e:
            r.capture_bitmap(BITMAP)                                 # no frame yet
        assert e.value.code == api.ERR_INVALID
        first = {"children": _content(w, h)}
        r.render(first)
        frame = r.read_image(premultiplied=True)
        assert len(np.unique(frame[..., 3])) > 8, "the frame holds many alphas"
        draw = {"children": [_whole_frame_bitmap(w, h, BITMAP)]}
        r.capture_bitmap(BITMAP)
        r.render(draw)
        assert diff_stats(r.read_image(premultiplied=True), frame) == (0, 0), "the captured bitmap drawn 1:1 is the frame"
        for bx, by in BOX_PAIRS:
            for passes in PASSES:
                r.render(first)
                r.capture_bitmap(BITMAP)
                r.blur_bitmap(BITMAP, bx, by, passes)
                r.render(draw)
                got = r.read_image(premultiplied=True)
                n, mx = diff_stats(got, bm.blur(frame, bx, by, passes))
                print("blur %dx%d box %dx%d passes %d: differing pixels %d max %d" % (w, h, bx, by, passes, n, mx))
                assert (n, mx) == (0, 0), (size, bx, by, passes)
        # blurring twice is blurring the blurred bitmap; a width of 0 is a width of 1
        r.blur_bitmap(BITMAP, 0, 2, 1)
        r.render(draw)
        bx, by = BOX_PAIRS[-1]
        assert diff_stats(r.read_image(premultiplied=True), bm.blur(bm.blur(frame, bx, by, PASSES[-1]), 1, 2, 1)) == (0, 0)
        with pytest.raises(api.SwfrError) as e:
            r.blur_bitmap(BITMAP + 1, 3, 3, 1)
        assert e.value.code == api.ERR_NOT_FOUND
        # a captured bitmap has no straight texels to transform
        with pytest.raises(api.SwfrError) as e:
            r.render({"children": [dict(draw["children"][0], color_transform={"red_mult": 0.5})]})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedCapturedBitmapTransform" in str(e.value)
    finally:
        r.close()


# ---- 2. a 1 x 1 box is the plain layer
def _layers_to_blurs(obj, count):
    if isinstance(obj, list):
        return [_layers_to_blurs(o, count) for o in obj]
    out = dict(obj)
    if out.get("layer") is not None and out.get("layer") is not False and out.get("mask") is None and out.get("opacity") is None:
        out["blur"] = {"x": 1, "y": 1}
        count[0] += 1
    if "children" in out:
        out["children"] = _layers_to_blurs(out["children"], count)
    return out


@pytest.mark.parametrize("aliased", (False, True), ids=("antialiased", "aliased"))
def test_a_1x1_box_is_the_plain_layer_overlap(aliased):
    gold = np.load(ls.golden_path("cairo_layer_aliased_overlap" if aliased else "cairo_layer_overlap"))
    scenes = ls.overlap_scenes()
    assert len(scenes) == 27
    for name, sc in sorted(scenes.items()):
        count = [0]
        stage = {"children": _layers_to_blurs(sc["stage"]["children"], count)}
        assert count[0] == 1, name
        got = dr.through_render(dict(sc, stage=stage), aliased)
        n, mx = diff_stats(got, gold[name])
        print("1x1", name, "aliased" if aliased else "", "differing pixels", n, "max", mx)
        assert (n, mx) == (0, 0), name


@pytest.mark.parametrize("mode", ls.MODES)
def test_a_1x1_box_is_the_plain_layer_sources(mode):
    gold = np.load(ls.golden_path("cairo_layer_sources_" + mode))
    done = 0
    for name, sc in sorted(ls.source_scenes(mode).items()):
        count = [0]
        stage = {"children": _layers_to_blurs(sc["stage"]["children"], count)}
        if not sc["exact"] or not 1 <= count[0] <= api.MAX_BLUR_LAYERS:
            continue
        r = dr.renderer_for(sc, False)
        try:
            r.render(stage)
            n, mx = diff_stats(r.read_image(premultiplied=True), gold[name])
        finally:
            r.close()
        print("1x1", name, "differing pixels", n, "max", mx)
        assert (n, mx) == (0, 0), name
        done += 1
    assert done >= 6


# ---- 3. the goldens of libcairo + pixman
@pytest.mark.parametrize("fname", sorted(bl.files()))
def test_goldens_through_render(fname):
    dr.goldens_through_render_and_resident(FAMILY, fname)


def test_alpha_and_erase_blurred_layers():
    dr.alpha_and_erase(FAMILY, "cairo_blur_operators", "normal_clear", "normal_opaque")


# ---- 4. the routes not taken refuse by name
def test_refused_routes_and_the_handle_afterwards():
    sc = bl.operator_scenes()["multiply_opaque"]
    plain = dict(sc, stage={"children": bl.without_blur(sc["stage"]["children"])})
    dr.refused_routes(FAMILY, sc, plain, np.load(bl.golden_path("cairo_blur_operators"))["multiply_opaque"], dr.through_render(plain))
    for contiguous in (False, True):                                  # a band handle captures no bitmap either
        b = dr.renderer_for(sc, False, band_index=0, band_count=2, contiguous_bands=contiguous)
        try:
            b.render(plain["stage"])
            with pytest.raises(api.SwfrError) as e:
                b.capture_bitmap(BITMAP)
            assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedBlurBands" in str(e.value)
        finally:
            b.close()


# ---- 5. nothing of a blurred frame stays behind
def test_a_plain_frame_after_a_blurred_one_is_a_fresh_handles_frame():
    dr.plain_frame_after(FAMILY, ("two_layers", "box_wider_than_frame", "blur_mask_opacity"), "cairo_blur_boxes")


def _many(n=300):
    """a plain stage of enough children for the frame builder to build it in pieces on its worker threads"""
    return {"children": [bl._shape([(2 + i % 50, 2 + i % 31), (20 + i % 47, 6 + i % 29), (9 + i % 43, 30 + i % 19)],
                                   (i * 7 % 256, i * 13 % 256, i * 29 % 256, 90 + i % 160)) for i in range(n)]}


def test_a_large_plain_frame_after_a_blurred_one_on_every_route(monkeypatch):
    """a stage built in pieces never walks on the handle's own builder: the last frame's sub-frames must be gone all the same -- the
    routes that refuse blurred layers take the plain frame, render does not draw stale sub-frames, and all give a fresh handle's frame"""
    monkeypatch.setenv("SWFR_BUILD_THREADS", "4")
    blurred = bl.box_scenes()["two_layers"]
    plain = dict(blurred, stage=_many())
    fresh = dr.through_render(plain)
    assert fresh[..., 3].any()
    r = dr.renderer_for(blurred, False)
    try:
        for route in ("render", "render_batch", "render_sequence", "render_sequence_readback", "build_frame"):
            r.render(blurred["stage"])
            assert len(r.built_layers()) == 2
            if route == "build_frame":
                r.build_frame(plain["stage"])
                assert r.built_layers() == []
                continue
            if route == "render_batch":
                r.render_batch([plain["stage"], plain["stage"]])
            else:
                getattr(r, route)(plain["stage"] if route == "render" else [plain["stage"]])
            assert r.built_layers() == [], route
            assert diff_stats(r.read_image(premultiplied=True), fresh) == (0, 0), route
    finally:
        r.close()


def test_arrays_built_before_a_bitmap_was_blurred_are_refused_by_name():
    """a colour-transformed fill's arrays name a texture variant of the bitmap; once the bitmap is blurred it has no straight texels"""
    w, h = 40, 24
    r = dr.handle(w, h)
    try:
        rgba = np.random.default_rng(5).integers(0, 256, (h, w, 4), dtype=np.uint8)
        r.register_bitmap(BITMAP, w, h, rgba.tobytes())
        stage = {"children": [dict(_whole_frame_bitmap(w, h, BITMAP), color_transform={"red_mult": 0.5})]}
        arrays = r.build_frame(stage)
        assert any(s.kind == api.STYLE_BITMAP and s.bitmap >= api.VARIANT_BASE for s in arrays[2])
        r.render(stage)                                               # fine while the bitmap is as registered
        r.blur_bitmap(BITMAP, 3, 3, 1)
        with pytest.raises(api.SwfrError) as e:
            r.upload_edges(*arrays)
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NotImplementedCapturedBitmapTransform" in str(e.value)
        r.render({"children": [_whole_frame_bitmap(w, h, BITMAP)]})   # untransformed it draws
    finally:
        r.close()


def test_path_timing_after_a_plain_and_a_blurred_render():
    """swfr_last_path_timing reports the whole call and its device time, for a frame with blurred layers too (its sub-frames' time is
    in upload_host_ms: swfr.h), and render_sequence adds the frames' times up"""
    sc = bl.operator_scenes()["multiply_opaque"]
    plain = bl.without_blur(sc["stage"]["children"])
    r = dr.renderer_for(sc, False)
    try:
        for stage in ({"children": plain}, sc["stage"], {"children": plain}):
            r.render(stage)
            t = r.path_timing()
            assert t["total_ms"] > 0 and t["device_ms"] > 0 and t["build_ms"] > 0 and t["upload_host_ms"] > 0, t
            assert t["total_ms"] >= t["build_ms"] + t["upload_host_ms"], t
            assert t["h2d_bytes"] > 0, t
        _, acc = r.render_sequence([{"children": plain}] * 3)
        assert acc["total_ms"] > 0 and acc["device_ms"] > 0, acc
    finally:
        r.close()
